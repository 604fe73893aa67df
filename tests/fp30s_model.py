"""Exact-integer model of fp30s.hip.h / g1_30s.hip.h (Fp in 13 signed limbs of 30 bits, Montgomery radix 2^390, and the
addition chain of k_fbw_accum over it), in the manner of ntt_lazy_model.py.

Two things:
  * the arithmetic itself on Python integers, limb for limb what the header computes (mont_product, carry, the
    conversions), with the largest column sum it met — the host tests compare the compiled header against it;
  * a propagation of BOUNDS through mul, sqr, mul2 and every step of g1s::chain_add (both states, both signs — the sign
    only negates a limb, so one pass covers both — and the doubling): per-limb magnitude bounds and value intervals in
    multiples of p, from the documented inputs.  check_chain_add() fails if a column bound reaches 2^63, if an input of
    a carry pass can exceed 3 * 2^29, or if a value leaves the interval the next step or the state documents; it
    returns the largest column of every product for the header's comments and NOTES."""
from fractions import Fraction as Fr

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
L = 13
H = 1 << 29
MASK = (1 << 30) - 1
R = 1 << 390
PINV = 0x30003
SEEDS = [1 << 30] + [(1 << 30) - 1] * 12 + [H - 1] + [H] * 11  # by column, fp30s::seed
LIMIT = 1 << 63
# the intervals of CHAIN_XYZZ (g1_30s.hip.h), in multiples of p
BOUND_X = Fr(22, 10)
BOUND_YZ = Fr(55, 100)


def value(l):
    return sum(v << (30 * i) for i, v in enumerate(l))


def sext30(x):
    x &= MASK
    return x - (1 << 30) if x >= H else x


def centred(v):
    out = []
    for _ in range(L - 1):
        d = sext30(v)
        out.append(d)
        v = (v - d) >> 30
    return out + [v]


def unsigned(v):
    assert v >= 0
    return [(v >> (30 * i)) & MASK for i in range(L - 1)] + [v >> 360]


P_LIMBS = centred(P)
ONE = centred(R % P - (P if R % P > P // 2 else 0))


def carry(l):
    """fp30s::carry"""
    out, cf, b = [], 0, 0
    for i in range(L - 1):
        t = l[i] + cf + b
        assert -(1 << 31) <= t < 1 << 31
        out.append(sext30(t))
        cf, b = t >> 30, (t >> 29) & 1
    return out + [l[L - 1] + cf + b]


def lazy_split(v, rnd):
    """limbs of value v with limbs 0..11 anywhere in [-3 * 2^29, 3 * 2^29] (the sum of three centred terms)"""
    l = centred(v)
    for i in range(L - 1):
        k = rnd.choice([-1, 0, 0, 1])
        if abs(l[i] + k * (1 << 30)) <= 3 * H:
            l[i] += k << 30
            l[i + 1] -= k
    for i in range(L - 1):
        if abs(l[i]) > 3 * H:  # a unit that arrived from below
            k = 1 if l[i] > 0 else -1
            l[i] -= k << 30
            l[i + 1] += k
    assert value(l) == v and all(abs(x) <= 3 * H for x in l[:12])
    return l


def lazy_pair(v, rnd):
    """limbs of value v as A - Q of two centred values: limbs 0..11 in (-2^30, 2^30)"""
    q = centred(rnd.randrange(-P // 2, P // 2))
    a = centred(v + value(q))
    l = [x - y for x, y in zip(a, q)]
    assert value(l) == v and all(abs(x) < 1 << 30 for x in l[:12])
    return l


def mont_product(kind, ops):
    """fp30s::mul / sqr / mul2 on limb lists: (result limbs, largest |column sum| met)"""
    if kind == "sqr":
        pairs = [(ops[0], ops[0])]
    elif kind == "mul2":
        pairs = [(ops[0], ops[1]), (ops[2], ops[3])]
    else:
        pairs = [(ops[0], ops[1])]
    m, r, acc, worst = [], [], 0, 0
    for k in range(2 * L - 1):
        lo, hi = max(0, k - L + 1), min(k, L - 1)
        acc += SEEDS[k]
        for a, b in pairs:
            acc += sum(a[i] * b[k - i] for i in range(lo, hi + 1))
        acc -= sum(m[i] * P_LIMBS[k - i] for i in range(lo, min(hi, len(m) - 1) + 1))
        worst = max(worst, abs(acc))
        if k < L:
            m.append(sext30((acc & 0xffffffff) * PINV))
            acc -= m[k] * P_LIMBS[0]
            worst = max(worst, abs(acc))
            assert acc & MASK == 0
        else:
            r.append((acc & MASK) - H)
        acc >>= 30
    assert worst < LIMIT
    return r + [acc], worst


def worst_case_products():
    """(kind, operands, why): limbs 0..11 at +(2^29 - 1) / -2^29 in the sign patterns that put every product of a column
    on one side; the top limbs at the largest the callers' values allow"""
    top = 1 << 25
    lo, hi = [-H] * 12, [H - 1] * 12
    u = [MASK] * 12
    alt = [(-H if i & 1 else H - 1) for i in range(12)]
    cases = []
    for a in (lo, hi, alt):
        for b in (lo, hi, alt):
            for ta in (-top, top):
                cases.append(("mul", [a + [ta], b + [-ta]], "extreme centred limbs"))
        for ta in (-top, top):
            cases.append(("sqr", [a + [ta]], "extreme centred limbs"))
            cases.append(("mul_u", [u + [top], a + [ta]], "unsigned first operand"))
    for a, b, c, d in ((lo, lo, lo, lo), (hi, hi, hi, hi), (lo, lo, hi, hi), (lo, hi, lo, hi), (alt, alt, alt, alt), (lo, hi, hi, lo)):
        for t in (-top, top):
            cases.append(("mul2", [a + [t], b + [t], c + [-t], d + [t]], "both products of one sign"))
    return cases


# ---- bounds ----
class B:
    """an operand known only by bounds: lim[i] = (least, greatest) limb i, lo < value / p < hi"""

    def __init__(self, lim, lo, hi):
        self.lim, self.lo, self.hi = list(lim), Fr(lo), Fr(hi)

    @property
    def mag(self):
        return max(abs(self.lo), abs(self.hi))


def with_top(least, greatest, lo, hi):
    """limbs 0..11 in [least, greatest]: the top limb is what the value leaves"""
    unit = sum(1 << (30 * i) for i in range(L - 1))
    top_lo = (int(Fr(lo) * P) - 1 - greatest * unit) >> 360
    top_hi = ((int(Fr(hi) * P) + 1 - least * unit) >> 360) + 1
    return B([(least, greatest)] * 12 + [(top_lo, top_hi)], lo, hi)


def b_centred(lo, hi):
    return with_top(-H, H - 1, lo, hi)


def b_lin(terms, cap):
    """sum of c * operand, limb-wise; cap is the largest limb magnitude the consumer admits"""
    lim = []
    for i in range(L):
        lim.append((sum(c * (t.lim[i][0] if c > 0 else t.lim[i][1]) for c, t in terms),
                    sum(c * (t.lim[i][1] if c > 0 else t.lim[i][0]) for c, t in terms)))
    worst = max(max(-l, h) for l, h in lim[:12])
    assert worst <= cap, "a limb can reach %d, over %d" % (worst, cap)
    assert all(-(1 << 31) <= l and h < (1 << 31) for l, h in lim), "int32"
    return B(lim, sum(c * (t.lo if c > 0 else t.hi) for c, t in terms), sum(c * (t.hi if c > 0 else t.lo) for c, t in terms))


def b_carry(x):
    assert max(max(-l, h) for l, h in x.lim[:12]) <= 3 * H, "carry pass input over 3 * 2^29"
    assert max(-x.lim[12][0], x.lim[12][1]) < 1 << 30
    return b_centred(x.lo, x.hi)


def _absprod(a, b):
    return max(abs(a[0] * b[0]), abs(a[0] * b[1]), abs(a[1] * b[0]), abs(a[1] * b[1]))


def b_product(pairs, report, name):
    """mul (one pair), sqr (the pair twice the same), mul2 (two pairs): column bounds, then the result's bounds"""
    import math
    worst, cin = 0, 0
    for k in range(2 * L - 1):
        lo, hi = max(0, k - L + 1), min(k, L - 1)
        col = SEEDS[k] + cin
        for a, b in pairs:
            col += sum(_absprod(a.lim[i], b.lim[k - i]) for i in range(lo, hi + 1))
        col += sum(H * abs(P_LIMBS[k - i]) for i in range(lo, hi + 1))
        worst = max(worst, col)
        cin = (col >> 30) + 1
    assert worst < LIMIT, "%s: a column can reach 2^%.2f" % (name, math.log2(worst))
    report[name] = max(report.get(name, 0), worst)
    extent = sum(max(abs(a.lo * b.lo), abs(a.lo * b.hi), abs(a.hi * b.lo), abs(a.hi * b.hi)) for a, b in pairs)
    lo = -extent if len(pairs) > 1 or pairs[0][0] is not pairs[0][1] else 0
    half = Fr(1, 2) + Fr(1, 1 << 28)  # |m| <= 2^389 (1 + 2^-29), against 2^390
    return b_centred(lo * P / R - half, extent * P / R + half)


def check_chain_add():
    """bounds through g1s::chain_add in CHAIN_AFFINE, CHAIN_XYZZ, the doubling and to_xyzz28; {product: largest column}"""
    rep = {}
    tab = with_top(0, MASK, 0, 1)          # from28 of a canonical table coordinate ("unsigned": limbs below 2^30)
    for state in ("affine", "xyzz"):
        if state == "affine":
            x1 = tab
            y1 = b_centred(-2, 2)
            zz1 = zzz1 = b_centred(-Fr(1, 2), Fr(1, 2))  # one()
            y2c = b_carry(tab)
            p = b_carry(b_lin([(1, tab), (-1, x1)], 3 * H))
            r = b_carry(b_lin([(2, y2c), (-1, y1)], 3 * H))
        else:
            x1 = with_top(-MASK, MASK, -BOUND_X, BOUND_X)
            y1 = b_centred(-BOUND_YZ, BOUND_YZ)
            zz1 = zzz1 = b_centred(-BOUND_YZ, BOUND_YZ)
            u2 = b_product([(tab, zz1)], rep, "U2 = x2 * ZZ1")
            s2 = b_product([(tab, zzz1)], rep, "S2 = y2 * ZZZ1")
            p = b_carry(b_lin([(1, u2), (-1, x1)], 3 * H))
            r = b_carry(b_lin([(2, s2), (-1, y1)], 3 * H))
        pp = b_product([(p, p)], rep, "PP = P^2")
        ppp = b_product([(p, pp)], rep, "PPP = P * PP")
        q = b_product([(x1, pp)], rep, "Q = X1 * PP")
        rr = b_product([(r, r)], rep, "RR = R^2")
        a = b_carry(b_lin([(1, rr), (-1, ppp), (-1, q)], 3 * H))
        x3 = b_lin([(1, a), (-1, q)], (1 << 30) - 1)
        v = b_carry(b_lin([(2, q), (-1, a)], 3 * H))
        y3 = b_product([(r, v), (y1, ppp)], rep, "Y3 = R * V - Y1 * PPP")
        zz3 = b_product([(zz1, pp)], rep, "ZZ3 = ZZ1 * PP")
        zzz3 = b_product([(zzz1, ppp)], rep, "ZZZ3 = ZZZ1 * PPP")
        assert x3.mag < BOUND_X and max(y3.mag, zz3.mag, zzz3.mag) < BOUND_YZ, state
        rep["|X3|/p, " + state] = float(x3.mag)
        rep["|Y3|/p, " + state] = float(y3.mag)
    # the doubling: x2 centred in [0, 1), y2 = +-2 y centred
    x2, y2 = b_carry(tab), b_centred(-2, 2)
    u = b_carry(b_lin([(2, y2)], 3 * H))
    zz = b_product([(u, u)], rep, "dbl: ZZ = U^2")
    zzz = b_product([(zz, u)], rep, "dbl: ZZZ")
    s = b_product([(x2, zz)], rep, "dbl: S")
    m = b_product([(x2, x2)], rep, "dbl: M")
    m3 = b_carry(b_lin([(3, m)], 3 * H))
    x3 = b_carry(b_lin([(1, b_product([(m3, m3)], rep, "dbl: M^2")), (-2, s)], 3 * H))
    y3 = b_product([(m3, b_carry(b_lin([(1, s), (-1, x3)], 3 * H))), (zzz, y2)], rep, "dbl: Y3")
    assert x3.mag < BOUND_X and max(y3.mag, zz.mag, zzz.mag) < BOUND_YZ
    # the way back: a product by a constant each, plus p
    k = b_centred(-Fr(1, 2), Fr(1, 2))
    for name, c in (("X", with_top(-MASK, MASK, -BOUND_X, BOUND_X)), ("Y", b_centred(-2, 2)), ("ZZ", b_centred(-BOUND_YZ, BOUND_YZ))):
        o = b_product([(c, k)], rep, "to_xyzz28: " + name)
        assert o.lo + 1 > 0 and o.hi + 1 < 2
    # the stand-alone rules of the header
    c = b_centred(-64, 64)
    b_product([(c, c)], rep, "mul, centred operands below 64p")
    b_product([(with_top(-MASK - 1, MASK + 1, -64, 64), c)], rep, "mul, first operand with limbs up to 2^30")
    b_product([(c, c), (c, c)], rep, "mul2, centred operands below 64p")
    return rep


if __name__ == "__main__":
    import math
    for k, v in check_chain_add().items():
        print("%-50s %s" % (k, "2^%.2f" % math.log2(v) if isinstance(v, int) else "%.3f" % v))
