"""A Python-integer model of the device pairing (rust-kzg_amd/csrc/fp12w.hip.h, pairing.hip): the tower, the line tables,
the Miller loop and the final exponentiation, formula for formula as the device code has them, which has them as
host_pairing.h has them.

Values are EXACT integers, not residues: a device register holds limbs whose value is an integer, wmul4 is the exact
Montgomery product (a*b + m*p) / 2^392, a padded subtraction adds K*p, so the model predicts the integer every result
register must hold — the device harness (tests/device_checks/pairing_check.hip) is compared value for value, and
verdicts (is the final value 1 mod p) are compared with the product's host code.  Every routine asserts the value
preconditions the header documents; the case generator builds operands at those bounds."""
import random

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
RBITS = 392
RMASK = (1 << RBITS) - 1
RW = (1 << RBITS) % P            # the Montgomery one
PINV = pow(P, -1, 1 << RBITS)
BLS_X_ABS = 0xd201000000010000
L = 14
LIMB = 1 << 28
FROM_BLST = (1 << 400) % P       # x * 2^384 -> x * 2^392 under wmul

SLOT_WORDS, NSLOTS, LINE_STEPS, LINE_WORDS = 192, 10, 68, 64
TABLE_WORDS, FROB_WORDS, PAIR_WORDS = LINE_STEPS * LINE_WORDS, 192, 48
OP_END, OP_ONE, OP_MUL, OP_SQR, OP_CSQR, OP_CONJ, OP_FROB, OP_INV, OP_LINE = range(9)
OP_NAMES = {OP_ONE: "one", OP_MUL: "f12_mul", OP_SQR: "f12_sqr", OP_CSQR: "f12_cyclotomic_sqr", OP_CONJ: "f12_conj",
            OP_FROB: "f12_frobenius", OP_INV: "f12_inv", OP_LINE: "line_step"}


def insn(op, d, a, b=0):
    return op | d << 8 | a << 16 | b << 24


# ---------------------------------------------------------------- Fp, as the device computes it
def wmul(a, b):
    """wmul4: operands up to ~1000p, result < a*b / 2^392 + p"""
    assert 0 <= a < 1000 * P and 0 <= b < 1000 * P
    t = a * b
    return (t + ((-t * PINV) & RMASK) * P) >> RBITS


def subk(K, a, b):
    """wsubk<K>: the subtrahend at most (K-1)p"""
    assert 0 <= b <= (K - 1) * P, "subtrahend of wsubk<%d> above %dp" % (K, K - 1)
    return a + K * P - b


def neg8(a):
    return subk(8, 0, a)


def reduce_(vals):
    for v in vals:
        assert v < 2520 * P
    return [wmul(v, RW) for v in vals]


def winv(a):
    assert a < 50 * P
    t = [0, wmul(a, RW)]
    for k in range(2, 16):
        t.append(wmul(t[k - 1], t[1]))
    e = P - 2
    acc = t[1]
    for j in range(94, -1, -1):
        for _ in range(4):
            acc = wmul(acc, acc)
        d = (e >> (4 * j)) & 15
        if d:
            acc = wmul(acc, t[d])
    return acc


# ---------------------------------------------------------------- Fp2 = (c0, c1), Fp6 = (c0, c1, c2), Fp12 = (c0, c1)
def f2_add(a, b):
    return (a[0] + b[0], a[1] + b[1])


def f2_sub(K, a, b):
    return (subk(K, a[0], b[0]), subk(K, a[1], b[1]))


def f2_mul_xi(K, a):
    return (subk(K, a[0], a[1]), a[0] + a[1])


def f2_muln(xs, ys):
    out = []
    for a, b in zip(xs, ys):
        assert (a[0] + a[1]) * (b[0] + b[1]) < 2520 * P * P, "an Fp2 product outside the 2p product bound"
        t0, t1, t2 = wmul(a[0], b[0]), wmul(a[1], b[1]), wmul(a[0] + a[1], b[0] + b[1])
        r = (subk(8, t0, t1), subk(8, t2, t0 + t1))
        assert r[0] < 10 * P and r[1] < 10 * P
        out.append(r)
    return out


def f6_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f6_sub(K, a, b):
    return tuple(f2_sub(K, x, y) for x, y in zip(a, b))


def f6_mul_v(K, a):
    return (f2_mul_xi(K, a[2]), a[0], a[1])


def f6_mul_pre(a, b):
    return ([a[0], a[1], a[2], f2_add(a[1], a[2]), f2_add(a[0], a[1]), f2_add(a[0], a[2])],
            [b[0], b[1], b[2], f2_add(b[1], b[2]), f2_add(b[0], b[1]), f2_add(b[0], b[2])])


def f6_mul_post(t):
    s12 = f2_sub(32, t[3], f2_add(t[1], t[2]))
    s01 = f2_sub(32, t[4], f2_add(t[0], t[1]))
    s02 = f2_sub(32, t[5], f2_add(t[0], t[2]))
    return (f2_add(t[0], f2_mul_xi(64, s12)), f2_add(s01, f2_mul_xi(32, t[2])), f2_add(s02, t[1]))


def flat(a):
    return [a[0][0][0], a[0][0][1], a[0][1][0], a[0][1][1], a[0][2][0], a[0][2][1],
            a[1][0][0], a[1][0][1], a[1][1][0], a[1][1][1], a[1][2][0], a[1][2][1]]


def unflat(v):
    return (((v[0], v[1]), (v[2], v[3]), (v[4], v[5])), ((v[6], v[7]), (v[8], v[9]), (v[10], v[11])))


def f6_flat(a):
    return [a[0][0], a[0][1], a[1][0], a[1][1], a[2][0], a[2][1]]


def f6_unflat(v):
    return ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))


def is_rform(a):
    return all(0 <= v < 2 * P for v in flat(a))


def f12_reduce(a):
    return unflat(reduce_(flat(a)))


def f6_reduce(a):
    return f6_unflat(reduce_(f6_flat(a)))


def f12_mul(a, b):
    assert is_rform(a) and is_rform(b)
    x0, y0 = f6_mul_pre(a[0], b[0])
    x1, y1 = f6_mul_pre(a[1], b[1])
    x2, y2 = f6_mul_pre(f6_add(a[0], a[1]), f6_add(b[0], b[1]))
    t = f2_muln(x0 + x1 + x2, y0 + y1 + y2)
    t0, t1, m = f6_mul_post(t[0:6]), f6_mul_post(t[6:12]), f6_mul_post(t[12:18])
    return f12_reduce((f6_add(t0, f6_mul_v(128, t1)), f6_sub(512, m, f6_add(t0, t1))))


def f12_sqr(a):
    assert is_rform(a)
    x0, y0 = f6_mul_pre(a[0], a[1])
    x1, y1 = f6_mul_pre(f6_add(a[0], a[1]), f6_add(a[0], f6_mul_v(8, a[1])))
    t = f2_muln(x0 + x1, y0 + y1)
    ab, m = f6_mul_post(t[0:6]), f6_mul_post(t[6:12])
    return f12_reduce((f6_sub(512, m, f6_add(ab, f6_mul_v(128, ab))), f6_add(ab, ab)))


def f12_cyclotomic_sqr(f):
    assert is_rform(f)
    za = [f[0][0], f[1][0], f[0][1]]
    zb = [f[1][1], f[0][2], f[1][2]]
    xs, ys = [], []
    for i in range(3):
        xs += [za[i], f2_add(za[i], zb[i])]
        ys += [zb[i], f2_add(za[i], f2_mul_xi(8, zb[i]))]
    t = f2_muln(xs, ys)
    r0 = [f2_sub(64, t[2 * i + 1], f2_add(t[2 * i], f2_mul_xi(32, t[2 * i]))) for i in range(3)]
    r1 = [f2_add(t[2 * i], t[2 * i]) for i in range(3)]

    def three_minus_two(tt, z):
        d = f2_sub(8, tt, z)
        return f2_add(f2_add(d, d), tt)

    def three_plus_two(tt, z):
        s = f2_add(tt, z)
        return f2_add(f2_add(s, s), tt)

    c00 = three_minus_two(r0[0], za[0])
    c11 = three_plus_two(r1[0], zb[0])
    c10 = three_plus_two(f2_mul_xi(32, r1[2]), za[1])
    c02 = three_minus_two(r0[2], zb[1])
    c01 = three_minus_two(r0[1], za[2])
    c12 = three_plus_two(r1[1], zb[2])
    return f12_reduce(((c00, c01, c02), (c10, c11, c12)))


def mul_ab0_pre(f, a2, b2):
    return [f[0], f[1], f2_add(f[0], f[1]), f[2], f[2]], [a2, b2, f2_add(a2, b2), b2, a2]


def mul_ab0_post(t):
    return (f2_add(t[0], f2_mul_xi(32, t[3])), f2_sub(32, t[2], f2_add(t[0], t[1])), f2_add(t[1], t[4]))


def f12_mul_line(f, a, b, cy):
    assert is_rform(f) and a[0] < 2 * P and a[1] < 2 * P and max(b) <= 8 * P and cy <= 8 * P
    bc = (b[0] + cy, b[1])
    x0, y0 = mul_ab0_pre(f[0], a, b)
    x1, y1 = mul_ab0_pre(f6_add(f[0], f[1]), a, bc)
    t = f2_muln(x0 + x1, y0 + y1)
    t0, m = mul_ab0_post(t[0:5]), mul_ab0_post(t[5:10])
    pr = [wmul(v, cy) for v in (f[1][2][0], f[1][2][1], f[1][0][0], f[1][0][1], f[1][1][0], f[1][1][1])]
    t1 = (f2_mul_xi(8, (pr[0], pr[1])), (pr[2], pr[3]), (pr[4], pr[5]))
    return f12_reduce((f6_add(t0, f6_mul_v(8, t1)), f6_sub(64, m, f6_add(t0, t1))))


def f12_conj(a):
    assert is_rform(a)
    n = tuple((neg8(x[0]), neg8(x[1])) for x in a[1])
    return (a[0], f6_reduce(n))


def f12_frobenius(a, frob):
    assert is_rform(a)
    ins = [a[0][0], a[1][0], a[0][1], a[1][1], a[0][2], a[1][2]]
    t = f2_muln([(x[0], neg8(x[1])) for x in ins], frob)
    return f12_reduce(((t[0], t[2], t[4]), (t[1], t[3], t[5])))


def f12_inv(a):
    assert is_rform(a)
    x0, y0 = f6_mul_pre(a[0], a[0])
    x1, y1 = f6_mul_pre(a[1], a[1])
    t = f2_muln(x0 + x1, y0 + y1)
    s0, s1 = f6_mul_post(t[0:6]), f6_mul_post(t[6:12])
    n = f6_reduce(f6_sub(512, s0, f6_mul_v(128, s1)))
    t = f2_muln([n[0], n[1], n[2], n[0], n[1], n[0]], [n[0], n[2], n[2], n[1], n[1], n[2]])
    abc = f6_reduce((f2_sub(64, t[0], f2_mul_xi(32, t[1])), f2_sub(32, f2_mul_xi(32, t[2]), t[3]), f2_sub(32, t[4], t[5])))
    t = f2_muln([n[0], n[2], n[1]], [abc[0], abc[1], abc[2]])
    s = f2_add(t[0], f2_mul_xi(32, f2_add(t[1], t[2])))
    fv = reduce_(list(s))
    ni = winv(wmul(fv[0], fv[0]) + wmul(fv[1], fv[1]))
    fi = (wmul(fv[0], ni), neg8(wmul(fv[1], ni)))
    d = f6_reduce(tuple(f2_muln([abc[0], abc[1], abc[2]], [fi, fi, fi])))
    x0, y0 = f6_mul_pre(a[0], d)
    x1, y1 = f6_mul_pre(a[1], d)
    t = f2_muln(x0 + x1, y0 + y1)
    r0, r1 = f6_mul_post(t[0:6]), f6_mul_post(t[6:12])
    zero = ((0, 0), (0, 0), (0, 0))
    return f12_reduce((r0, f6_sub(128, zero, r1)))


def f12_one():
    return unflat([RW] + [0] * 11)


def f12_is_one(a):
    v = flat(a)
    return (v[0] - RW) % P == 0 and all(x % P == 0 for x in v[1:])


# ---------------------------------------------------------------- the G2 side: plain arithmetic mod p (host work)
def g2f_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def g2f_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def g2f_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * n % P, -a[1] * n % P)


G2_GEN = ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
           0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
          (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
           0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be))


def g2_double(Q):
    x, y = Q
    x2 = g2f_mul(x, x)
    lam = g2f_mul((3 * x2[0] % P, 3 * x2[1] % P), g2f_inv((2 * y[0] % P, 2 * y[1] % P)))
    nx = g2f_sub(g2f_mul(lam, lam), (2 * x[0] % P, 2 * x[1] % P))
    return (nx, g2f_sub(g2f_mul(lam, g2f_sub(x, nx)), y))


def g2_line_table(Q):
    """Q = (x, y) affine on the twist, plain residues, or None: the 68 (lambda, c) of host_pairing.h's g2_line_table"""
    if Q is None:
        return None
    tx, ty = Q
    tab = []
    for bit in range(62, -1, -1):
        x2 = g2f_mul(tx, tx)
        lam = g2f_mul((3 * x2[0] % P, 3 * x2[1] % P), g2f_inv((2 * ty[0] % P, 2 * ty[1] % P)))
        tab.append((lam, g2f_sub(g2f_mul(lam, tx), ty)))
        nx = g2f_sub(g2f_mul(lam, lam), (2 * tx[0] % P, 2 * tx[1] % P))
        ty = g2f_sub(g2f_mul(lam, g2f_sub(tx, nx)), ty)
        tx = nx
        if (BLS_X_ABS >> bit) & 1:
            lam = g2f_mul(g2f_sub(Q[1], ty), g2f_inv(g2f_sub(Q[0], tx)))
            tab.append((lam, g2f_sub(g2f_mul(lam, tx), ty)))
            ax = g2f_sub(g2f_sub(g2f_mul(lam, lam), tx), Q[0])
            ty = g2f_sub(g2f_mul(lam, g2f_sub(tx, ax)), ty)
            tx = ax
    assert len(tab) == LINE_STEPS
    return tab


def table_mont(tab):
    """the device table's values: lambda.c0, lambda.c1, c.c0, c.c1 per step, canonical, radix 2^392"""
    return None if tab is None else [tuple(v * RW % P for v in (lam[0], lam[1], c[0], c[1])) for lam, c in tab]


def g2_affine_from_jacobian_mont384(words72):
    """a blst_p2 (72 words, Montgomery 2^384) -> affine plain (x, y) or None for infinity (z == 0)"""
    inv384 = pow(1 << 384, -1, P)
    co = [sum(words72[12 * k + i] << (32 * i) for i in range(12)) * inv384 % P for k in range(6)]
    x, y, z = (co[0], co[1]), (co[2], co[3]), (co[4], co[5])
    if all(sum(words72[12 * k + i] for i in range(12)) == 0 for k in (4, 5)):
        return None
    zi = g2f_inv(z)
    zi2 = g2f_mul(zi, zi)
    return (g2f_mul(x, zi2), g2f_mul(y, g2f_mul(zi2, zi)))


def frobenius_constants():
    """g[k] = xi^(k (p-1)/6), canonical, radix 2^392, as Fp2 pairs"""
    def f2pow(a, e):
        r = (1, 0)
        for bit in bin(e)[2:]:
            r = g2f_mul(r, r)
            if bit == "1":
                r = g2f_mul(r, a)
        return r
    g1 = f2pow((1, 1), (P - 1) // 6)
    g = [(1, 0)]
    for _ in range(5):
        g.append(g2f_mul(g[-1], g1))
    return [(a * RW % P, b * RW % P) for a, b in g]


FROB = frobenius_constants()


# ---------------------------------------------------------------- the program and the interpreter
def build_program(miller=True, final=True):
    F, T0, T1, T2, T3, T4, T5, T6, A, B = range(10)
    p = []
    if miller:
        p.append(insn(OP_ONE, F, 0))
        idx = 0
        for bit in range(62, -1, -1):
            p.append(insn(OP_SQR, F, F))
            p.append(insn(OP_LINE, F, F, idx))
            idx += 1
            if (BLS_X_ABS >> bit) & 1:
                p.append(insn(OP_LINE, F, F, idx))
                idx += 1
        p.append(insn(OP_CONJ, F, F))

    def exp_x(d, a):
        for bit in range(62, -1, -1):
            p.append(insn(OP_CSQR, d, a if bit == 62 else d))
            if (BLS_X_ABS >> bit) & 1:
                p.append(insn(OP_MUL, d, d, a))
        p.append(insn(OP_CONJ, d, d))

    if final:
        p += [insn(OP_CONJ, A, F), insn(OP_INV, B, F), insn(OP_MUL, T2, A, B), insn(OP_FROB, A, T2), insn(OP_FROB, A, A),
              insn(OP_MUL, T2, A, T2), insn(OP_CSQR, T1, T2), insn(OP_CONJ, T1, T1)]
        exp_x(T3, T2)
        p += [insn(OP_CSQR, T4, T3), insn(OP_MUL, T5, T1, T3)]
        exp_x(T1, T5)
        exp_x(T0, T1)
        exp_x(A, T0)
        p.append(insn(OP_MUL, T6, A, T4))
        exp_x(T4, T6)
        p += [insn(OP_CONJ, T5, T5), insn(OP_MUL, A, T5, T2), insn(OP_MUL, T4, T4, A), insn(OP_CONJ, T5, T2),
              insn(OP_MUL, T1, T1, T2), insn(OP_FROB, T1, T1), insn(OP_FROB, T1, T1), insn(OP_FROB, T1, T1),
              insn(OP_MUL, A, T6, T5), insn(OP_FROB, T6, A), insn(OP_MUL, A, T3, T0), insn(OP_FROB, A, A),
              insn(OP_FROB, T3, A), insn(OP_MUL, A, T3, T1), insn(OP_MUL, A, A, T6), insn(OP_MUL, F, A, T4)]
    p.append(insn(OP_END, 0, 0))
    return p


class Pairs:
    """per pair: z3, xz, y (R-form, y <= 8p for the negated side), the Montgomery table or None, skip"""
    def __init__(self):
        self.z3, self.xz, self.y, self.tab, self.skip = [0, 0], [0, 0], [0, 0], [None, None], [True, True]


def line_step(f, pr, step):
    for k in range(2):
        if pr.skip[k]:
            continue
        l0, l1, c0, c1 = pr.tab[k][step]
        t = [wmul(c0, pr.z3[k]), wmul(c1, pr.z3[k]), wmul(l0, pr.xz[k]), wmul(l1, pr.xz[k])]
        f = f12_mul_line(f, (t[0], t[1]), (neg8(t[2]), neg8(t[3])), pr.y[k])
    return f


def run_program(prog, slots, pr, frob=None):
    frob = FROB if frob is None else frob
    for w in prog:
        op, d, a, b = w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24
        if op == OP_END:
            break
        if op == OP_ONE:
            r = f12_one()
        elif op == OP_MUL:
            r = f12_mul(slots[a], slots[b])
        elif op == OP_SQR:
            r = f12_sqr(slots[a])
        elif op == OP_CSQR:
            r = f12_cyclotomic_sqr(slots[a])
        elif op == OP_CONJ:
            r = f12_conj(slots[a])
        elif op == OP_FROB:
            r = f12_frobenius(slots[a], frob)
        elif op == OP_INV:
            r = f12_inv(slots[a])
        else:
            assert op == OP_LINE
            r = line_step(slots[a], pr, b)
        assert is_rform(r), "the result of %s is not in R-form" % OP_NAMES[op]
        slots[d] = r
    return slots


def pairs_prepare(a1_words, b1_words, tabs):
    """a1, b1: blst_p1 as 36 words (Jacobian, Montgomery 2^384, any 384-bit values); tabs: two Montgomery tables or None"""
    pr = Pairs()
    for k, w in enumerate((a1_words, b1_words)):
        X, Y, Z = (wmul(sum(w[12 * c + i] << (32 * i) for i in range(12)), FROM_BLST) for c in range(3))
        pr.tab[k] = tabs[k]
        pr.skip[k] = tabs[k] is None or Z % P == 0
        zz, xz = wmul(Z, Z), wmul(X, Z)
        pr.z3[k], pr.xz[k] = wmul(zz, Z), xz
        pr.y[k] = neg8(Y) if k == 0 else Y
    return pr


ZERO12 = unflat([0] * 12)


def pairing_check(a1_words, b1_words, tabs, prog=None):
    """the verdict of k_pairing_check and the final value"""
    pr = pairs_prepare(a1_words, b1_words, tabs)
    if pr.skip[0] and pr.skip[1]:
        return True, None
    slots = run_program(prog or FULL_PROGRAM, [ZERO12] * NSLOTS, pr)
    return f12_is_one(slots[0]), slots[0]


FULL_PROGRAM = build_program()


# ---------------------------------------------------------------- limb forms for the device harness
def limbs_canonical(v):
    """14 limbs, 0..12 below 2^28 (the top limb takes what is left)"""
    assert 0 <= v < 1 << (28 * 13 + 31)
    return [(v >> (28 * i)) & (LIMB - 1) for i in range(13)] + [v >> (28 * 13)]


def limbs_loose(v, rng):
    """an N-form of v with some limbs exactly 2^28: a zero limb under a non-zero one borrows from it"""
    l = limbs_canonical(v)
    for i in range(12, -1, -1):
        if l[i] == 0 and l[i + 1] > 0 and rng.random() < 0.75:
            l[i] = LIMB
            l[i + 1] -= 1
    assert sum(x << (28 * i) for i, x in enumerate(l)) == v and all(x <= LIMB for x in l[:13])
    return l


def words16(l):
    return list(l) + [0, 0]


def value_of(words):
    """a row of 16 device words -> (value, ok) where ok says limbs 0..12 <= 2^28 and lanes 14, 15 zero"""
    ok = all(w <= LIMB for w in words[:13]) and words[14] == 0 and words[15] == 0
    return sum(w << (28 * i) for i, w in enumerate(words[:14])), ok


def slot_words(a, rng=None):
    out = []
    for v in flat(a):
        out += words16(limbs_loose(v, rng) if rng else limbs_canonical(v))
    return out


# ---------------------------------------------------------------- cases for the device harness
UNIT_PROG = 8
UNIT_NIN = UNIT_PROG + 2 + 3 * SLOT_WORDS + 2 * PAIR_WORDS + 2 * LINE_WORDS + FROB_WORDS
UNIT_NOUT = 12 * 64
PAIRING_PROG = 768
PAIRING_NIN = 72 + 2 + 2 * TABLE_WORDS + FROB_WORDS + 1 + PAIRING_PROG
PAIRING_NOUT = SLOT_WORDS + 3
OPS = {"unit": (UNIT_NIN, UNIT_NOUT), "pairing": (PAIRING_NIN, PAIRING_NOUT), "winv": (16, 64)}


def frob_words():
    out = []
    for a, b in FROB:
        out += words16(limbs_canonical(a)) + words16(limbs_canonical(b))
    return out


def table_words(tab):
    if tab is None:
        return [0] * TABLE_WORDS
    out = []
    for e in tab:
        for v in e:
            out += words16(limbs_canonical(v))
    return out


class UnitCase:
    """one operation on slots 1, 2 (3 unused): the result register of all 64 lanes against the model's integers"""

    def __init__(self, tag, op, a, b=None, pr=None, rng=None):
        self.tag, self.op = tag, op
        b = b if b is not None else ZERO12
        pr = pr or Pairs()
        prog = [insn(op, 0, 1, 2 if op == OP_MUL else 0), insn(OP_END, 0, 0)]
        self.expect = flat(run_program(prog, [ZERO12, a, b] + [ZERO12] * 7, pr)[0])
        w = prog + [0] * (UNIT_PROG - len(prog)) + [int(pr.skip[0]), int(pr.skip[1])]
        w += slot_words(a, rng) + slot_words(b, rng) + slot_words(ZERO12)
        for k in range(2):
            for v in (pr.z3[k], pr.xz[k], pr.y[k]):
                w += words16(limbs_loose(v, rng) if rng else limbs_canonical(v))
        for k in range(2):
            e = pr.tab[k][0] if pr.tab[k] else (0, 0, 0, 0)
            for v in e:
                w += words16(limbs_canonical(v))
        w += frob_words()
        assert len(w) == UNIT_NIN
        self.words = w

    def check(self, out):
        assert len(out) == UNIT_NOUT
        for k in range(12):
            for row in range(4):
                v, ok = value_of(out[64 * k + 16 * row:64 * k + 16 * row + 16])
                assert ok, "coefficient %d row %d: limbs not in N-form or lanes 14, 15 not zero" % (k, row)
                assert v == self.expect[k], "coefficient %d row %d: value differs from the model" % (k, row)
                assert v < 2 * P


class PairingCase:
    """two G1 points and two tables through a program (the whole check, or the Miller loop alone): slot 0 and the verdict"""

    def __init__(self, tag, a1, b1, tabs, prog=None):
        self.tag = tag
        prog = prog or FULL_PROGRAM
        assert len(prog) <= PAIRING_PROG
        pr = pairs_prepare(a1, b1, tabs)
        self.skips = [int(pr.skip[0]), int(pr.skip[1])]
        self.slot0 = flat(run_program(prog, [ZERO12] * NSLOTS, pr)[0])
        self.verdict = int(f12_is_one(unflat(self.slot0)))
        w = list(a1) + list(b1) + [int(tabs[0] is not None), int(tabs[1] is not None)]
        w += table_words(tabs[0]) + table_words(tabs[1]) + frob_words() + [len(prog)] + prog + [0] * (PAIRING_PROG - len(prog))
        assert len(w) == PAIRING_NIN
        self.words = w

    def check(self, out):
        assert len(out) == PAIRING_NOUT
        assert out[SLOT_WORDS + 1:] == self.skips, "skipped pairs differ"
        for k in range(12):
            v, ok = value_of(out[16 * k:16 * k + 16])
            assert ok and v == self.slot0[k], "coefficient %d of slot 0 differs from the model" % k
        assert out[SLOT_WORDS] == self.verdict, "verdict differs"


class WinvCase:
    """the Fp inversion alone: a N-form, value < 50p; the result in all four rows, R-form, a * result = 1 unless a = 0 mod p"""

    def __init__(self, tag, a, rng=None):
        assert 0 <= a < 50 * P
        self.tag, self.a, self.expect = tag, a, winv(a)
        assert self.expect < 2 * P and (a * self.expect * pow(RW, -2, P) - (1 if a % P else 0)) % P == 0
        self.words = words16(limbs_loose(a, rng) if rng else limbs_canonical(a))

    def check(self, out):
        assert len(out) == 64
        for row in range(4):
            v, ok = value_of(out[16 * row:16 * row + 16])
            assert ok, "row %d: limbs not in N-form or lanes 14, 15 not zero" % row
            assert v == self.expect, "row %d: value differs from the model" % row


def winv_cases(rng, n=12):
    cases = [WinvCase("zero", 0), WinvCase("p in limb form", P), WinvCase("one", RW), WinvCase("just under 50p", 50 * P - 1, rng),
             WinvCase("49p: 0 mod p at the bound", 49 * P), WinvCase("limbs at 2^28", 1 << 364, rng)]
    return cases + [WinvCase("random %d" % i, rng.randrange(50 * P), rng if i % 2 else None) for i in range(n)]


def rand_rform(rng):
    return unflat([rng.randrange(2 * P) for _ in range(12)])


def const12(v):
    return unflat([v] * 12)


def cyclotomic_element(rng):
    """a random element of the cyclotomic subgroup: f^((p^6-1)(p^2+1)) by the model's own easy part"""
    f = rand_rform(rng)
    t = f12_mul(f12_conj(f), f12_inv(f))
    return f12_mul(f12_frobenius(f12_frobenius(t, FROB), FROB), t)


def unit_cases(rng, per_op=24):
    """every tower routine: random, at the upper bound of the value (2p - 1) and of the limbs (2^28), zero, one, and 0 mod p
    as p itself"""
    top, pp, one = const12(2 * P - 1), const12(P), f12_one()
    loose = const12(1 << 364)  # below p; its loose form has every limb 0..11 at 2^28
    special = [("upper bound", top), ("zero", ZERO12), ("one", one), ("p in limb form", pp), ("limbs at 2^28", loose)]
    cases = []
    for op in (OP_MUL, OP_SQR, OP_CSQR, OP_CONJ, OP_FROB, OP_INV):
        name = OP_NAMES[op]
        for tag, a in special:
            for tag2, b in (special if op == OP_MUL else [("", None)]):
                cases.append(UnitCase("%s %s %s" % (name, tag, tag2), op, a, b, rng=rng))
        n = per_op if op != OP_INV else 4
        for i in range(n):
            a = cyclotomic_element(rng) if op == OP_CSQR and i % 2 else rand_rform(rng)
            b = rand_rform(rng) if op == OP_MUL else None
            cases.append(UnitCase("%s random %d" % (name, i), op, a, b, rng=rng if i % 2 else None))
    # the line step: table entries canonical, z3 / xz R-form, y up to 8p; either pair skipped, both, none
    for i in range(per_op):
        pr = Pairs()
        for k in range(2):
            hi = i % 4 == 0
            pr.z3[k] = 2 * P - 1 if hi else rng.randrange(2 * P)
            pr.xz[k] = 2 * P - 1 if hi else rng.randrange(2 * P)
            pr.y[k] = 8 * P if hi else rng.randrange(8 * P + 1)
            pr.tab[k] = [tuple(P - 1 if hi else rng.randrange(P) for _ in range(4))]
            pr.skip[k] = bool((i >> (2 + k)) & 1) if i >= 4 else False
        a = top if i % 4 == 0 else rand_rform(rng)
        cases.append(UnitCase("line_step %d skip %s" % (i, pr.skip), OP_LINE, a, None, pr=pr, rng=rng))
    return cases


def p1_words(pt, z=1):
    """affine (x, y) or None -> the 36 words of a blst_p1 (Jacobian, Montgomery 2^384) with the given Z"""
    if pt is None:
        return [0] * 36
    out = []
    for v in (pt[0] * z * z % P, pt[1] * z * z * z % P, z % P):
        m = v * (1 << 384) % P
        out += [(m >> (32 * i)) & 0xffffffff for i in range(12)]
    return out


def pairing_cases():
    """8 checks: e([6]G, G2) against e([3]G, [2]G2) and its neighbours, with Z != 1, infinity, a missing table, a curve
    point outside G1, and the Miller loop alone"""
    import g1_encodings as E

    tg = table_mont(g2_line_table(G2_GEN))
    t2 = table_mont(g2_line_table(g2_double(G2_GEN)))
    g3, g4, g6 = E.mul(3, E.G), E.mul(4, E.G), E.mul(6, E.G)
    outside = E.torsion_point(11)
    cases = [PairingCase("true", p1_words(g6), p1_words(g3, 12345), [tg, t2]),
             PairingCase("false", p1_words(g6, 99), p1_words(g4), [tg, t2]),
             PairingCase("miller loop alone", p1_words(g6, 99), p1_words(g4), [tg, t2], prog=build_program(final=False)),
             PairingCase("a1 at infinity", p1_words(None), p1_words(g4), [tg, t2]),
             PairingCase("both at infinity", p1_words(None), p1_words(None), [tg, t2]),
             PairingCase("b2 the identity", p1_words(g3), p1_words(g4), [tg, None]),
             PairingCase("outside G1", p1_words(outside, 7), p1_words(g3), [tg, t2]),
             PairingCase("true, swapped tables", p1_words(g3, 5), p1_words(g6, 3), [t2, tg])]
    assert [c.verdict for c in cases] == [1, 0, 0, 0, 1, 0, 0, 1]
    return cases


def encode(blocks):
    parts = []
    for op, cases in blocks.items():
        parts.append("%s %d\n" % (op, len(cases)))
        parts += [" ".join("%x" % w for w in c.words) + "\n" for c in cases]
    return "".join(parts)


def decode(text, blocks):
    lines = text.split("\n")
    pos = 0
    outs = {}
    for op, cases in blocks.items():
        assert lines[pos] == "%s %d" % (op, len(cases)), "block header %r, expected %s %d" % (lines[pos][:80], op, len(cases))
        pos += 1
        got = []
        for _ in cases:
            words = [int(x, 16) for x in lines[pos].split()]
            assert len(words) == OPS[op][1], "%s: %d words in a line, expected %d" % (op, len(words), OPS[op][1])
            got.append(words)
            pos += 1
        outs[op] = got
    assert lines[pos] == "done", "no end marker"
    return outs


def failures(blocks, outs):
    bad = []
    for op, cases in blocks.items():
        for i, (c, o) in enumerate(zip(cases, outs[op])):
            try:
                c.check(o)
            except AssertionError as e:
                bad.append((op, i, "%s: %s" % (c.tag, e)))
    return bad
