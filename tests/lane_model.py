"""Python-integer model, case generators and checkers for the lane-parallel arithmetic (fpw.hip.h, g1w.hip.h,
g1grp.hip.h) and for the single-lane routines of g1_28.hip.h at the boundary between the two (points the wide code
stored).  Shared by tests/test_lane_arith_gpu.py (runs tests/device_checks/lane_check.hip on the GPU) and
tests/test_lane_arith_cases_cpu.py (builds the cases, checks the model against the oracle, runs the single-lane cases on
the host).  Nothing here calls the library.

A case is (op, input words, checker): the checker takes the words the harness printed for the case and raises
AssertionError.  Every generator asserts the preconditions of the routine it feeds — the bounds written in the header
above that routine — so an out-of-contract input is a bug in this file, not a finding about the device code.
"""
import os
import random

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
L = 14
W = 28
M28 = (1 << W) - 1
FULL = 1 << W                 # the limb value wnorm may leave ("limbs <= 2^28")
R = 1 << (L * W)              # Montgomery radix 2^392
RINV = pow(R, -1, P)
SENTINEL = 0xA5A5A5A5
TOP_SHIFT = W * (L - 1)       # 364

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------ field, limbs
def value(limbs):
    return sum(x << (W * i) for i, x in enumerate(limbs))


def limbs_strict(v):
    """the normalized form: limbs 0..12 < 2^28, the rest in the top limb"""
    assert 0 <= v < 1 << (TOP_SHIFT + 32)
    return [(v >> (W * i)) & M28 for i in range(L - 1)] + [v >> TOP_SHIFT]


def is_strict(limbs):
    return len(limbs) == L and all(0 <= x <= M28 for x in limbs[:L - 1]) and 0 <= limbs[L - 1] < 1 << 32


def is_wide_normal(limbs):
    return len(limbs) == L and all(0 <= x <= FULL for x in limbs[:L - 1]) and 0 <= limbs[L - 1] < 1 << 32


def with_full_limbs(v, positions):
    """A wide-normal form with limb i == 2^28 for every i in positions: the value is v with those (strict) limbs
    cleared — never larger than v — and one unit borrowed from the limb above each.  Returns the limbs."""
    l = limbs_strict(v)
    for i in positions:
        assert 0 <= i < L - 1
        l[i] = 0
    v2 = value(l)
    for i in sorted(positions):
        l[i] += FULL
        l[i + 1] -= 1
    if any(x < 0 for x in l):  # a borrow from an empty limb: the strict form of the same value
        return limbs_strict(v2)
    assert value(l) == v2 and is_wide_normal(l)
    return l


def to_mont(x):
    return x * R % P


def from_mont(v):
    return v * RINV % P


def edge_values(k, rnd, nrandom=12):
    """values in [0, k*p): the multiples of p and their neighbours, an empty top limb, the maximum, random ones"""
    out = [0, 1, k * P - 1, (1 << TOP_SHIFT) - 1, 1 << TOP_SHIFT, M28, FULL]
    for j in range(k):
        out += [j * P, j * P + 1, max(0, j * P - 1)]
    out += [rnd.randrange(k * P) for _ in range(nrandom)] + [rnd.randrange(1 << TOP_SHIFT) for _ in range(3)]
    return [v for v in out if v < k * P]


# ------------------------------------------------------------------------------------------------ curve
B_COEFF = 4


def on_curve(pt):
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - B_COEFF) % P == 0


def aff_neg(a):
    return None if a is None else (a[0], (-a[1]) % P)


def aff_dbl(a):
    if a is None or a[1] == 0:
        return None
    s = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    x = (s * s - 2 * a[0]) % P
    return (x, (s * (a[0] - x) - a[1]) % P)


def aff_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        return aff_dbl(a) if a[1] == b[1] else None
    s = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (s * s - a[0] - b[0]) % P
    return (x, (s * (a[0] - x) - a[1]) % P)


def aff_mul(k, a):
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = aff_dbl(acc)
        if bit == "1":
            acc = aff_add(acc, a)
    return acc


def decompress(hex48):
    b = bytes.fromhex(hex48)
    assert len(b) == 48 and b[0] & 0x80
    if b[0] & 0x40:
        return None
    x = int.from_bytes(b, "big") & ((1 << 381) - 1)
    y = pow((x ** 3 + B_COEFF) % P, (P + 1) // 4, P)
    assert (y * y - x ** 3 - B_COEFF) % P == 0, "not on the curve"
    if (y > P - y) != bool(b[0] & 0x20):
        y = P - y
    return (x, y)


def compress(pt):
    if pt is None:
        return (0xc0 << 376).to_bytes(48, "big").hex()
    v = pt[0] | (1 << 383) | ((1 << 381) if pt[1] > P - pt[1] else 0)
    return v.to_bytes(48, "big").hex()


def generator():
    """[tau^0] G1 of the monomial setup in tests/golden/trusted_setup.txt: the generator"""
    with open(os.path.join(HERE, "golden", "trusted_setup.txt")) as f:
        lines = f.read().split()
    n1, n2 = int(lines[0]), int(lines[1])
    g = decompress(lines[2 + n1 + n2])
    assert g is not None and on_curve(g)
    return g


_points = {}


def sample_points():
    """multiples of the generator: small ones and large ones"""
    if not _points:
        g = generator()
        rnd = random.Random(381)
        ks = [1, 2, 3, 5, 7, 8, 64, 65] + [rnd.randrange(1 << 250, 1 << 254) for _ in range(10)]
        _points["g"] = g
        _points["pts"] = [aff_mul(k, g) for k in ks]
        assert all(p is not None and on_curve(p) for p in _points["pts"])
    return _points["pts"]


# ------------------------------------------------------------------------------------------------ XYZZ / Jacobian
COORDS = ("x", "y", "zzz", "zz")  # g1::Xyzz in memory


class Rep:
    """a point as four (or three) integer coordinate values in Montgomery form, any representative"""

    def __init__(self, x, y, zzz, zz):
        self.x, self.y, self.zzz, self.zz = x, y, zzz, zz

    def values(self):
        return [self.x, self.y, self.zzz, self.zz]


INF = Rep(0, 0, 0, 0)


def lift(pt, z, jx=0, jy=0, jzzz=0, jzz=0):
    """affine -> XYZZ with ZZ = z^2, ZZZ = z^3 in Montgomery form, coordinates shifted to x + j*p"""
    if pt is None:
        return Rep(0, 0, 0, 0)
    z %= P
    assert z != 0
    zz, zzz = z * z % P, z * z * z % P
    return Rep(to_mont(pt[0] * zz) + jx * P, to_mont(pt[1] * zzz) + jy * P, to_mont(zzz) + jzzz * P, to_mont(zz) + jzz * P)


def affine_of(x, y, zzz, zz):
    """the affine point four coordinate VALUES represent (None for ZZ == 0 mod p), with ZZ^3 == ZZZ^2 checked"""
    if zz % P == 0:
        return None
    a, b = from_mont(zz), from_mont(zzz)
    assert (a ** 3 - b * b) % P == 0, "ZZ^3 != ZZZ^2"
    return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)


def point_words_limbs(limbs4):
    assert len(limbs4) == 4 and all(len(l) == L for l in limbs4)
    return [w for l in limbs4 for w in l]


# ------------------------------------------------------------------------------------------------ wave output parsing
def split_rows(reg):
    """64 words of a wide register -> four rows of 14 limbs; lanes 14 and 15 of every row must hold zero"""
    assert len(reg) == 64
    rows = []
    for r in range(4):
        row = reg[16 * r:16 * r + 16]
        assert row[14] == 0 and row[15] == 0, "lane 14/15 of row %d not zero: %x %x" % (r, row[14], row[15])
        rows.append(row[:14])
    return rows


def replicated(reg):
    """64 words of a wide register whose four rows must hold the same value -> its 14 limbs"""
    rows = split_rows(reg)
    for r in range(1, 4):
        assert rows[r] == rows[0], "row %d differs from row 0" % r
    return rows[0]


def wreg(rows):
    """input words of a wide register from four rows of 14 limbs"""
    assert len(rows) == 4 and all(len(r) == L and all(0 <= x < 1 << 32 for x in r) for r in rows)
    return [w for r in rows for w in r]


def wrep(limbs):
    return wreg([limbs] * 4)


class Case:
    __slots__ = ("op", "words", "check", "tag")

    def __init__(self, op, words, check, tag=""):
        self.op, self.words, self.check, self.tag = op, list(words), check, tag


OPS = {}  # op -> (words in, words out), as tests/device_checks/lane_check.hip has them
PT = 56
GRP_OUT = 1 + PT
ADD_N_SLOTS = 13
CHAIN_STEPS, CHAIN_OPERANDS = 64, 8
STORE_GUARD = 8
for _name, _nin, _nout in [
        ("wnorm", 56, 64), ("wnorm_full", 56, 64), ("wsqr", 56, 64), ("waddn", 112, 64), ("wsub16", 112, 64), ("wsub32", 112, 64),
        ("wmul4", 112, 64), ("wdbl", 168, 192), ("wide_roundtrip", 14, 64 * 15), ("is_zero", 56, 64),
        ("load_store", PT, 256 + 2 * STORE_GUARD + PT + 64 * PT), ("dbl", PT, 256), ("dadd", 2 * PT, 256), ("dbl_k", PT + 1, 256),
        ("add_n", PT + 2 + ADD_N_SLOTS * PT, 256), ("chain", PT + 1 + CHAIN_OPERANDS * PT + 2 * CHAIN_STEPS, CHAIN_STEPS * 256),
        ("grp_dbl1", PT, GRP_OUT), ("grp_dbl2", PT, 2 * GRP_OUT), ("grp_dbl4", PT, 4 * GRP_OUT),
        ("grp_dadd1", 2 * PT, GRP_OUT), ("grp_dadd2", 2 * PT, 2 * GRP_OUT), ("grp_dadd4", 2 * PT, 4 * GRP_OUT),
        ("grp_madd4", PT + 28, 4 * GRP_OUT), ("one_dadd", 2 * PT, GRP_OUT), ("one_dadd_unequal", 2 * PT, GRP_OUT),
        ("one_dbl_k", PT + 1, GRP_OUT), ("one_madd", PT + 28, GRP_OUT), ("one_chain_add", PT + 2 + 28, GRP_OUT),
        ("one_to_blst", PT, GRP_OUT), ("one_reduce_xy", PT, GRP_OUT)]:
    OPS[_name] = (_nin, _nout)


# ------------------------------------------------------------------------------------------------ fpw cases
def wnorm_inputs(rnd):
    """limbs < 2^31 (wnorm's stated input bound), the top limb included"""
    top = 0x1a011
    ins = [
        [0] * L,
        [(1 << 31) - 1] * L,
        [FULL] + [M28] * 12 + [top],                       # the longest ripple: a carry from limb 0 to the top limb
        [M28] + [M28] * 12 + [top],                        # its neighbours: no carry at all,
        [FULL + 1] + [M28] * 12 + [top],                   # one more at the bottom,
        [FULL] + [M28] * 5 + [M28 - 1] + [M28] * 6 + [top],  # a ripple that stops half way,
        [FULL] + [M28] * 11 + [M28 - 1, top],              # and one that stops a limb below the top
        [0, FULL] + [M28] * 11 + [top],
        [FULL] * 13 + [top],                               # the non-strict form wnorm may leave
        [FULL] * 13 + [0],
        [0, 1 << 29, FULL - 2] + [M28] * 10 + [top],       # a ripple that only starts after the first carry round
        [(1 << 31) - 1] * 13 + [0],
        [0] * 13 + [(1 << 31) - 1],
    ]
    for _ in range(43):
        bits = rnd.choice([28, 29, 30, 31])
        ins.append([rnd.randrange(1 << bits) if rnd.random() < 0.8 else (1 << bits) - 1 for _ in range(L)])
    for l in ins:
        assert len(l) == L and all(0 <= x < 1 << 31 for x in l)
    return ins


def _rows_case(op, in_regs_rows, check_row, tag=""):
    """in_regs_rows: per input register four rows; check_row(r, out_row)"""
    words = []
    for rows in in_regs_rows:
        words += wreg(rows)

    def chk(out):
        rows = split_rows(out[:64])
        for r in range(4):
            try:
                check_row(r, rows[r])
            except AssertionError as e:
                raise AssertionError("row %d: %s" % (r, e))

    return Case(op, words, chk, tag)


def wnorm_cases(rnd, full):
    ins = wnorm_inputs(rnd)
    while len(ins) % 4:
        ins.append(ins[2])
    cases = []
    for i in range(0, len(ins), 4):
        rows = ins[i:i + 4]

        def check_row(r, out, rows=rows):
            assert value(out) == value(rows[r]), "value changed"
            if full:
                assert all(x < FULL for x in out[:13]), "limbs 0..12 not < 2^28"
            else:
                assert all(x <= FULL for x in out[:13]), "limbs 0..12 not <= 2^28"

        cases.append(_rows_case("wnorm_full" if full else "wnorm", [rows], check_row))
    return cases


def wide_normal_operands(k, rnd):
    """wide-normal forms (limbs <= 2^28 inclusive) of values below k*p: the edges in strict form (the only wide-normal form
    a value without an empty limb has), forms with limbs equal to 2^28, and the form with EVERY limb at 2^28"""
    out = [limbs_strict(v) for v in edge_values(k, rnd)]
    for _ in range(10):
        v = rnd.randrange(k * P // 2, k * P)
        out.append(with_full_limbs(v, rnd.sample(range(0, 12, 2), rnd.randrange(1, 6))))
    top = (k * P >> TOP_SHIFT) - 2
    if top >= 0:
        out.append([FULL] * 13 + [top])
    out.append(with_full_limbs(k * P - 1, [0]))
    for l in out:
        assert is_wide_normal(l) and value(l) < k * P
    return out


def waddsub_cases(rnd):
    """waddn, wsub16 (b < 15p), wsub32 (b < 31p): a within the limb bound that keeps the sum below wnorm's 2^31 — the pad
    limbs are below 3 * 2^28, so a's limbs may reach 5 * 2^28 - 1 (2^31 - 2^28 - 1 for waddn) —, b wide-normal"""
    cases = []
    for op, kb, pad, amax in (("waddn", 18, 0, (1 << 31) - FULL - 1), ("wsub16", 15, 16, 5 * FULL - 1), ("wsub32", 31, 32, 5 * FULL - 1)):
        bs = wide_normal_operands(kb, rnd)
        pairs = []
        for b in bs:
            a = rnd.choice([
                [0] * L, limbs_strict(rnd.randrange(2 * P)), limbs_strict(rnd.randrange(18 * P)), [amax] * 13 + [1 << 29],
                [rnd.randrange(amax + 1) for _ in range(13)] + [rnd.randrange(1 << 29)],
                [x + y for x, y in zip(limbs_strict(rnd.randrange(2 * P)), limbs_strict(rnd.randrange(2 * P)))]])
            assert all(x <= amax for x in a[:13]) and a[13] <= 1 << 29
            pairs.append((a, b))
        pairs.append(([amax] * 13 + [1 << 29], bs[0]))
        pairs.append(([0] * L, limbs_strict(kb * P - 1)))
        while len(pairs) % 4:
            pairs.append(pairs[-1])
        for i in range(0, len(pairs), 4):
            four = pairs[i:i + 4]

            def check_row(r, out, four=four, pad=pad, op=op):
                a, b = four[r]
                want = value(a) + value(b) if op == "waddn" else value(a) + pad * P - value(b)
                assert value(out) == want, "value identity (a limb wrapped?)"
                assert all(x <= FULL for x in out[:13]), "not normalized"

            cases.append(_rows_case(op, [[p[0] for p in four], [p[1] for p in four]], check_row))
    return cases


# the value pairs the g1w formulas form (in units of p), and one just under 2^392 * p = 2520.5.. p^2
WMUL_PAIRS = [(2, 2), (18, 18), (36, 36), (34, 34), (6, 34), (18, 2), (63, 40)]


def wmul_operand_pairs(rnd):
    """operand pairs for wmul4: limbs < 2^29, a * b < 2^392 * p (fp28::mul's product bound)"""
    pairs = []
    for ka, kb in WMUL_PAIRS:
        pairs.append((limbs_strict(ka * P - 1), limbs_strict(kb * P - 1)))
        pairs.append((limbs_strict(kb * P - 1), limbs_strict(ka * P - 1)))
        ea, eb = edge_values(ka, rnd, 3), edge_values(kb, rnd, 3)
        for _ in range(6):
            pairs.append((limbs_strict(rnd.choice(ea)), limbs_strict(rnd.choice(eb))))
    for k in range(0, 37):  # k*p and its neighbours against a value below 2p (and against itself up to 36p)
        for v in (k * P, k * P + 1, max(k * P - 1, 0)):
            pairs.append((limbs_strict(v), limbs_strict(rnd.choice([P - 1, P, P + 1, 2 * P - 1, rnd.randrange(2 * P)]))))
        pairs.append((limbs_strict(k * P), limbs_strict(k * P)))
    for _ in range(20):  # an empty top limb, on one side and on both
        a, b = rnd.randrange(1 << TOP_SHIFT), rnd.randrange(1 << TOP_SHIFT)
        pairs.append((limbs_strict(a), limbs_strict(rnd.randrange(18 * P))))
        pairs.append((limbs_strict(a), limbs_strict(b)))
    pairs.append((limbs_strict((1 << TOP_SHIFT) - 1), limbs_strict((1 << TOP_SHIFT) - 1)))
    for _ in range(30):  # lazy sums of two normalized values
        a = [x + y for x, y in zip(limbs_strict(rnd.randrange(18 * P)), limbs_strict(rnd.randrange(18 * P)))]
        b = [x + y for x, y in zip(limbs_strict(rnd.randrange(18 * P)), limbs_strict(rnd.randrange(18 * P)))]
        pairs.append((a, b))
    for _ in range(10):  # wide-normal forms with limbs equal to 2^28, and two of them added
        a = with_full_limbs(rnd.randrange(9 * P, 18 * P), rnd.sample(range(0, 12, 2), 3))
        b = with_full_limbs(rnd.randrange(9 * P, 18 * P), rnd.sample(range(1, 12, 2), 3))
        pairs.append((a, b))
        pairs.append(([x + y for x, y in zip(a, b)], b))  # full limbs at different positions: sums stay below 2^29
    for top in (0x1a011, 0):
        allfull = [FULL] * 13 + [top]
        pairs.append((allfull, allfull))
        pairs.append(([2 * x - 1 for x in allfull[:13]] + [top], limbs_strict(2 * P - 1)))
    big = [(1 << 29) - 1] * L  # every limb at the bound: the other operand as large as the product bound leaves
    bmax = (R * P - 1) // value(big)
    pairs += [(big, limbs_strict(bmax)), (limbs_strict(bmax), big), (big, limbs_strict(rnd.randrange(bmax))), (big, [0] * L),
              (big, limbs_strict(1))]
    half = [(1 << 29) - 1] * 7 + [0] * 7  # both operands with every limb at the bound, in the low half
    pairs.append((half, half))
    for a, b in pairs:
        assert len(a) == L and len(b) == L and all(0 <= x < 1 << 29 for x in a + b), "limb bound"
        assert value(a) * value(b) < R * P, "product bound"
    return pairs


def check_mont_row(prod):
    def chk(out):
        assert all(x <= FULL for x in out[:13]), "limbs 0..12 not <= 2^28"
        assert value(out) < 2 * P, "value not below 2p"
        assert (value(out) - prod * RINV) % P == 0, "wrong residue"

    return chk


def wmul_cases(rnd):
    pairs = wmul_operand_pairs(rnd)
    rnd.shuffle(pairs)
    while len(pairs) % 4:
        pairs.append(pairs[0])
    cases = []
    for i in range(0, len(pairs), 4):
        four = pairs[i:i + 4]

        def check_row(r, out, four=four):
            check_mont_row(value(four[r][0]) * value(four[r][1]))(out)

        cases.append(_rows_case("wmul4", [[p[0] for p in four], [p[1] for p in four]], check_row))
    return cases


def wsqr_cases(rnd):
    ops = [a for a, b in wmul_operand_pairs(rnd) if value(a) ** 2 < R * P] + [limbs_strict(50 * P)]
    assert all(value(a) ** 2 < R * P for a in ops)
    while len(ops) % 4:
        ops.append(ops[0])
    cases = []
    for i in range(0, len(ops), 4):
        four = ops[i:i + 4]

        def check_row(r, out, four=four):
            check_mont_row(value(four[r]) ** 2)(out)

        cases.append(_rows_case("wsqr", [four], check_row))
    return cases


def wmul_row_independence(rnd):
    """Four different pairs: each alone (replicated in the four rows), then all four at once in each of the four rotations.
    Returns the cases and a function of all their outputs: a pair's result must be, limb for limb, what it gives alone,
    in whichever row and beside whichever neighbours it runs."""
    pairs = [(limbs_strict(36 * P - 1), limbs_strict(36 * P - 1)), (limbs_strict(1), limbs_strict(1)),
             ([(1 << 29) - 1] * 7 + [0] * 7, [(1 << 29) - 1] * 7 + [0] * 7), (limbs_strict(rnd.randrange(18 * P)), limbs_strict(rnd.randrange(2 * P)))]
    cases, layout = [], []
    for i in range(4):
        layout.append([i] * 4)
    for s in range(4):
        layout.append([(r + s) % 4 for r in range(4)])
    for rows in layout:
        def check_row(r, out, rows=rows):
            a, b = pairs[rows[r]]
            check_mont_row(value(a) * value(b))(out)

        cases.append(_rows_case("wmul4", [[pairs[i][0] for i in rows], [pairs[i][1] for i in rows]], check_row))

    def cross_check(outs):
        alone = [split_rows(outs[i][:64])[0] for i in range(4)]
        for c, rows in enumerate(layout):
            got = split_rows(outs[c][:64])
            for r in range(4):
                assert got[r] == alone[rows[r]], "case %d row %d: pair %d does not give what it gives alone" % (c, r, rows[r])

    return cases, cross_check


def jac_lift(pt, z, jx, jy, jz):
    z %= P
    return [to_mont(pt[0] * z * z) + jx * P, to_mont(pt[1] * z * z * z) + jy * P, to_mont(z) + jz * P]


def wdbl_cases(rnd):
    """fpw::wdbl on Jacobian (X, Y, Z) at the boundary of its invariant X < 18p, Y < 17.1p, Z < 2.1p (normalized), which
    must hold again on the output"""
    bx, by, bz = 18 * P, 171 * P // 10, 21 * P // 10
    cases = []
    for n, pt in enumerate(sample_points()):
        for rep in range(3):
            z = rnd.randrange(1, P)
            if rep == 0:
                v = jac_lift(pt, z, 17, 16, 1)  # the largest representatives below the bounds
                for i, b in enumerate((bx, by, bz)):
                    while v[i] + P < b:
                        v[i] += P
            elif rep == 1:
                v = jac_lift(pt, z, 0, 0, 0)
            else:
                v = jac_lift(pt, z, rnd.randrange(18), rnd.randrange(17), rnd.randrange(2))
            limbs = [limbs_strict(x) for x in v]
            if rep == 2:  # Z = z R is any value one likes: a form with a limb equal to 2^28
                T, i = value_with_empty_limb(1, bz, rnd)
                v = jac_lift(pt, from_mont(T), rnd.randrange(18), rnd.randrange(17), 0)
                v[2] = T
                limbs = [limbs_strict(v[0]), limbs_strict(v[1]), with_full_limbs(T, [i])]
                assert limbs[2][i] == FULL
            assert v[0] < bx and v[1] < by and v[2] < bz and all(is_wide_normal(l) for l in limbs)
            vals = [value(l) for l in limbs]
            assert vals == v
            assert jac_affine(vals) == pt
            want = aff_dbl(pt)

            def chk(out, want=want):
                regs = [replicated(out[64 * i:64 * i + 64]) for i in range(3)]
                assert all(all(x <= FULL for x in l[:13]) for l in regs), "not normalized"
                X, Y, Z = (value(l) for l in regs)
                assert X < bx and Y < by and Z < bz, "invariant: X %.2fp Y %.2fp Z %.2fp" % (X / P, Y / P, Z / P)
                assert jac_affine([X, Y, Z]) == want, "wrong point"

            cases.append(Case("wdbl", wrep(limbs[0]) + wrep(limbs[1]) + wrep(limbs[2]), chk))
    return cases


def jac_affine(v):
    z = from_mont(v[2])
    if z == 0:
        return None
    zi = pow(z, -1, P)
    return (from_mont(v[0]) * zi * zi % P, from_mont(v[1]) * zi * zi * zi % P)


def roundtrip_cases(rnd):
    """to_wide -> from_wide: any 32-bit limbs"""
    ins = [[0] * L, [0xffffffff] * L, list(range(1, 15)), [FULL] * L] + [[rnd.randrange(1 << 32) for _ in range(L)] for _ in range(12)]
    cases = []
    for a in ins:
        def chk(out, a=a):
            assert replicated(out[:64]) == a, "to_wide"
            for k in range(L):
                assert out[64 * (1 + k):64 * (2 + k)] == [a[k]] * 64, "from_wide limb %d" % k

        cases.append(Case("wide_roundtrip", a, chk))
    return cases


def is_zero_cases(rnd):
    """g1w::is_zero_mod_p: a normalized (limbs <= 2^28) value below 64p.  k*p for every k < 64 and its neighbours; values
    that are no multiple of p but pass the filter (low limb == that of k*p, k < 64); forms with limbs equal to 2^28.
    (No k*p with 0 < k < 64 has an empty limb among limbs 0..12, so its strict form is its only wide-normal form: the
    2^28-limb forms here are of multiples made to have one — none exists — and of the neighbouring non-multiples.)"""
    ins = []
    for k in range(64):
        kp = limbs_strict(k * P)
        assert k == 0 or all(x != 0 for x in kp[:13])
        ins.append((kp, 1))
        ins.append((limbs_strict(k * P + 1), 0))
        if k:
            ins.append((limbs_strict(k * P - 1), 0))
        # the same low limb as k*p: passes the filter, fails the exact comparison
        for d in (1 << W, 1 << TOP_SHIFT, rnd.randrange(1, 1 << 200) << W, (rnd.randrange(1, P >> W) << W)):
            v = k * P + d
            if v < 64 * P:
                assert v % P != 0 and (v & M28) == (k * P & M28)
                ins.append((limbs_strict(v), 0))
    # limbs equal to 2^28: values = 0 mod 2^28 (filter digit 0) and their like
    ins.append(([FULL] + [0] * 13, 0))
    ins.append(([FULL] * 13 + [0], 0))
    ins.append(([FULL] * 13 + [0x1a011], 0))
    for _ in range(10):
        v = rnd.randrange(64 * P)
        l = with_full_limbs(v, rnd.sample(range(12), 2))
        ins.append((l, int(value(l) % P == 0)))
        l = with_full_limbs(v, [0])
        ins.append((l, int(value(l) % P == 0)))
    for _ in range(40):
        v = rnd.randrange(64 * P)
        ins.append((limbs_strict(v), int(v % P == 0)))
    cases = []
    for l, want in ins:
        assert is_wide_normal(l) and value(l) < 64 * P and want == int(value(l) % P == 0)

        def chk(out, want=want):
            assert out[:64] == [want] * 64, "answer %s, expected %d in every lane" % (sorted(set(out[:64])), want)

        cases.append(Case("is_zero", wrep(l), chk))
    return cases


# ------------------------------------------------------------------------------------------------ g1w cases
WIDE_BOUNDS = (18, 18, 2, 2)  # g1w.hip.h: X, Y < 18p, ZZZ, ZZ < 2p between calls (limbs <= 2^28)


def top_rep(v, k):
    """the largest representative of v (mod p) below k*p"""
    v %= P
    return v + (k * P - 1 - v) // P * P


def sqrt_mod_p(a):
    """a square root of a mod p, or None (p = 3 mod 4)"""
    r = pow(a % P, (P + 1) // 4, P)
    return r if r * r % P == a % P else None


def value_with_empty_limb(lo, hi, rnd):
    """a value in [lo, hi) whose strict form has limb i empty and limb i + 1 not: (value, i)"""
    while True:
        l = limbs_strict(rnd.randrange(lo, hi))
        i = rnd.randrange(12)
        l[i] = 0
        if l[i + 1] and value(l) >= lo:
            return value(l), i


def wide_reps(pt, rnd, which):
    """limbs of the four coordinates of pt under the bounds of g1w: which = 'low' (canonical residues), 'top' (the largest
    representatives under the bounds), 'mixed' (random representatives, and one coordinate — X or ZZ, the two a choice of
    z can set to a given value — in a form with a limb equal to 2^28)"""
    if pt is None:
        return [[0] * L] * 4
    full = None
    z = rnd.randrange(1, P)
    if which == "mixed":
        while True:  # z^2 = T / R (ZZ = T) or T / (x R) (X = T) for a target T with an empty limb: half of them are squares
            c = rnd.choice([0, 3])
            T, i = value_with_empty_limb(P if c == 0 else 0, WIDE_BOUNDS[c] * P, rnd)
            zz = from_mont(T) * (pow(pt[0], -1, P) if c == 0 else 1) % P
            z = sqrt_mod_p(zz)
            if z and (c == 3 or pt[0] != 0):
                full = (c, T, i)
                break
    vals = lift(pt, z).values()
    if which == "top":
        vals = [top_rep(v, k) for v, k in zip(vals, WIDE_BOUNDS)]
    elif which == "mixed":
        vals = [v + rnd.randrange(k) * P for v, k in zip(vals, WIDE_BOUNDS)]
    limbs = [limbs_strict(v) for v in vals]
    if full:
        c, T, i = full
        assert T % P == vals[c] % P
        limbs[c] = with_full_limbs(T, [i])
        assert limbs[c][i] == FULL and value(limbs[c]) == T
    for l, k in zip(limbs, WIDE_BOUNDS):
        assert is_wide_normal(l) and value(l) < k * P
    assert affine_of(*[value(l) for l in limbs]) == pt
    return limbs


def neg_reps(limbs, rnd, k_y):
    """-P from the limbs of P: Y replaced by k*p - Y for a k that keeps it in [0, k_y * p)"""
    y = value(limbs[1])
    ks = [k for k in range(1, k_y + 1) if 0 <= k * P - y < k_y * P]
    k = rnd.choice(ks)
    return [limbs[0], limbs_strict(k * P - y), limbs[2], limbs[3]]


def check_point_regs(regs, want, bounds, strict=False):
    """regs: limbs of x, y, zzz, zz; want: affine point or None"""
    for name, l in zip(COORDS, regs):
        lim = M28 if strict else FULL
        assert all(x <= lim for x in l[:13]), "%s not normalized" % name
        assert SENTINEL not in l, "%s holds an unwritten word" % name
    vals = [value(l) for l in regs]
    if want is None:
        assert all(x == 0 for x in regs[3]), "expected infinity (ZZ all-zero), ZZ = %x" % vals[3]
        return
    assert any(regs[3]), "infinity, expected a point"
    for name, v, k in zip(COORDS, vals, bounds):
        assert v < k * P, "%s = %.3f p, bound %d p" % (name, v / P, k)
    assert vals[3] % P != 0, "ZZ == 0 mod p"
    got = affine_of(*vals)
    assert got == want, "wrong point"


def check_wide_point(out256, want, bounds=WIDE_BOUNDS):
    regs = [replicated(out256[64 * i:64 * i + 64]) for i in range(4)]
    check_point_regs(regs, want, bounds)
    return regs


def pair_cases(rnd, reps_of, neg_ky):
    """(acc limbs, b limbs, expected point, tag) for an addition: ordinary and every exceptional case, with equal and with
    different z and representatives on the two sides"""
    pts = sample_points()
    out = []
    for i, p in enumerate(pts):
        q = pts[(i + 3) % len(pts)]
        for which in ("low", "top", "mixed"):
            a, b = reps_of(p, rnd, which), reps_of(q, rnd, rnd.choice(["low", "top", "mixed"]))
            out.append((a, b, aff_add(p, q), "P+Q"))
            out.append((reps_of(None, rnd, which), b, q, "inf+Q"))
            out.append((a, reps_of(None, rnd, which), p, "P+inf"))
            out.append((a, a, aff_dbl(p), "P+P same z"))
            out.append((a, reps_of(p, rnd, rnd.choice(["low", "top", "mixed"])), aff_dbl(p), "P+P other z"))
            out.append((a, neg_reps(a, rnd, neg_ky), None, "P+(-P) same z"))
            out.append((a, neg_reps(reps_of(p, rnd, rnd.choice(["low", "top", "mixed"])), rnd, neg_ky), None, "P+(-P) other z"))
        out.append((reps_of(None, rnd, "low"), reps_of(None, rnd, "low"), None, "inf+inf"))
    return out


def load_store_cases(rnd):
    """load -> store and to_single: any wide-normal coordinates (load does not look at them); store and to_single write the
    exactly normalized form of the same values, store 56 words and no more"""
    ins = []
    for pt in sample_points()[:6]:
        for which in ("low", "top", "mixed"):
            ins.append(wide_reps(pt, rnd, which))
    ins.append([[0] * L] * 4)
    ripple = [FULL] + [M28] * 12 + [0x1a011]
    ins.append([ripple, [FULL] * 13 + [0], [0, FULL] + [M28] * 11 + [5], ripple])
    cases = []
    for limbs in ins:
        assert all(is_wide_normal(l) for l in limbs)

        def chk(out, limbs=limbs):
            regs = [replicated(out[64 * i:64 * i + 64]) for i in range(4)]
            assert regs == [list(l) for l in limbs], "load"
            want = [limbs_strict(value(l)) for l in limbs]
            o = 256
            assert out[o:o + STORE_GUARD] == [SENTINEL] * STORE_GUARD, "store wrote in front of its slot"
            assert out[o + STORE_GUARD + PT:o + 2 * STORE_GUARD + PT] == [SENTINEL] * STORE_GUARD, "store wrote behind its slot"
            assert out[o + STORE_GUARD:o + STORE_GUARD + PT] == point_words_limbs(want), "store: not the exactly normalized value"
            o += 2 * STORE_GUARD + PT
            for lane in range(64):
                assert out[o + lane * PT:o + (lane + 1) * PT] == point_words_limbs(want), "to_single, lane %d" % lane

        cases.append(Case("load_store", point_words_limbs(limbs), chk))
    return cases


def dbl_cases(rnd):
    cases = []
    for pt in sample_points():
        for which in ("low", "top", "mixed"):
            limbs = wide_reps(pt, rnd, which)
            cases.append(Case("dbl", point_words_limbs(limbs), lambda out, w=aff_dbl(pt): check_wide_point(out[:256], w), which))
    return cases


def dadd_cases(rnd):
    cases = []
    for a, b, want, tag in pair_cases(rnd, wide_reps, 18):
        cases.append(Case("dadd", point_words_limbs(a) + point_words_limbs(b), lambda out, w=want: check_wide_point(out[:256], w), tag))
    return cases


DBL_KS = (0, 1, 2, 5, 64)


def dbl_k_cases(rnd):
    cases = []
    pts = sample_points()
    for i, pt in enumerate(pts + [None]):
        for k in DBL_KS:
            if k == 64 and i % 4:  # the long ones on a few points
                continue
            which = rnd.choice(["low", "top", "mixed"]) if k not in (1, 64) else "top"
            limbs = wide_reps(pt, rnd, which)
            want = pt
            for _ in range(k):
                want = aff_dbl(want)
            cases.append(Case("dbl_k", point_words_limbs(limbs) + [k], lambda out, w=want: check_wide_point(out[:256], w), "k=%d" % k))
    return cases


def add_n_cases(rnd):
    """acc += src[0] + src[stride] + ...: n = 1..5, stride 1 and 3, partial sums through infinity and through a doubling;
    the slots between and behind the operands hold other points"""
    pts = sample_points()
    cases = []
    it = 0
    for n in range(1, 6):
        for stride in (1, 3):
            for script in ("plain", "inf", "dbl", "from_inf"):
                it += 1
                p, q, s = pts[it % len(pts)], pts[(it + 5) % len(pts)], pts[(it + 9) % len(pts)]
                acc = p
                if script == "plain":
                    ops = [q, s, aff_dbl(q), p, aff_add(p, s)][:n]
                elif script == "inf":   # acc + (-acc) = infinity first, then on from there
                    ops = [aff_neg(p), q, q, aff_neg(aff_dbl(q)), s][:n]
                elif script == "dbl":   # acc + acc, then 2acc + 2acc
                    ops = [p, aff_dbl(p), q, aff_neg(q), None][:n]
                else:
                    acc = None
                    ops = [None, q, q, s, aff_neg(s)][:n]
                want = acc
                for o in ops:
                    want = aff_add(want, o)
                slots = [wide_reps(pts[(it + j) % len(pts)], rnd, "low") for j in range(ADD_N_SLOTS)]
                for j, o in enumerate(ops):
                    slots[j * stride] = wide_reps(o, rnd, rnd.choice(["low", "top", "mixed"]))
                words = point_words_limbs(wide_reps(acc, rnd, rnd.choice(["low", "top", "mixed"]))) + [n, stride]
                for sl in slots:
                    words += point_words_limbs(sl)
                cases.append(Case("add_n", words, lambda out, w=want: check_wide_point(out[:256], w), "n=%d stride=%d %s" % (n, stride, script)))
    return cases


def chain_cases(rnd, nchains=4):
    """scripted chains of 64 mixed dbl / dadd / dbl_k steps on one accumulator: the bounds and the point after every step"""
    pts = sample_points()
    cases = []
    for c in range(nchains):
        start = pts[(3 * c + 1) % len(pts)]
        q1, q2, q3 = pts[(3 * c + 2) % len(pts)], pts[(3 * c + 6) % len(pts)], pts[(3 * c + 11) % len(pts)]
        operands = [q1, aff_neg(q1), q2, start, aff_neg(start), None, q3, aff_dbl(q2)]
        acc, steps, wants = start, [], []
        for s in range(CHAIN_STEPS):
            if s == 0 and c % 2 == 0:
                choice = (1, 4)                       # start - start: through infinity at once
            elif s == 5:
                choice = (1, operands.index(None))
            else:
                kind = rnd.random()
                if acc is None:
                    choice = (1, rnd.choice([0, 2, 6]))
                elif kind < 0.3:
                    choice = (0, 0)
                elif kind < 0.45:
                    choice = (2, rnd.choice([1, 2, 3, 5]))
                elif kind < 0.55:                    # the accumulator's own value or its negative, when the table has it
                    same = [i for i, o in enumerate(operands) if o is not None and (o == acc or o == aff_neg(acc))]
                    choice = (1, rnd.choice(same)) if same else (1, rnd.randrange(8))
                else:
                    choice = (1, rnd.randrange(8))
            op, arg = choice
            if op == 0:
                assert acc is not None  # g1w::dbl: acc != infinity
                acc = aff_dbl(acc)
            elif op == 1:
                acc = aff_add(acc, operands[arg])
            else:
                for _ in range(arg):
                    acc = aff_dbl(acc)
            steps += [op, arg]
            wants.append(acc)
        if c % 2 == 0:
            assert None in wants
        words = point_words_limbs(wide_reps(start, rnd, "top")) + [CHAIN_STEPS]
        for o in operands:
            words += point_words_limbs(wide_reps(o, rnd, rnd.choice(["low", "top", "mixed"])))
        words += steps

        def chk(out, wants=wants, steps=steps):
            for s, w in enumerate(wants):
                try:
                    check_wide_point(out[256 * s:256 * s + 256], w)
                except AssertionError as e:
                    raise AssertionError("step %d (op %d %d): %s" % (s, steps[2 * s], steps[2 * s + 1], e))

        cases.append(Case("chain", words, chk))
    return cases


# ------------------------------------------------------------------------------------------------ grp / single-lane cases
ONE_BOUNDS = (10, 6, 2, 2)       # g1_28.hip.h: X < 10p, Y < 6p, ZZZ, ZZ < 2p
ONE_BOUNDS_NEG = (10, 8, 2, 2)   # dbl and dadd also take Y <= 8p (a negated input)


def one_reps_for(bounds):
    def reps(pt, rnd, which):
        if pt is None:
            return [[0] * L] * 4
        vals = lift(pt, rnd.randrange(1, P)).values()
        if which == "top":
            vals = [top_rep(v, k) for v, k in zip(vals, bounds)]
        elif which == "mixed":
            vals = [v + rnd.randrange(k) * P for v, k in zip(vals, bounds)]
        limbs = [limbs_strict(v) for v in vals]
        for l, k in zip(limbs, bounds):
            assert is_strict(l) and value(l) < k * P
        return limbs

    return reps


def check_group(out, G, check_lane):
    lanes = [out[GRP_OUT * r:GRP_OUT * (r + 1)] for r in range(G)]
    for r in range(1, G):
        assert lanes[r] == lanes[0], "lane %d of the group differs from lane 0" % r
    flag, words = lanes[0][0], lanes[0][1:]
    regs = [words[L * i:L * (i + 1)] for i in range(4)]
    check_lane(flag, regs)


def grp_place(cases, G):
    """every case at every group position of a quad in turn: the list is emitted 4 / G times, each time shifted by one
    more group (the filler in front is the list's first case)"""
    q = 4 // G
    out = []
    for s in range(q):
        for i, c in enumerate(cases):
            while len(out) % q != (i + s) % q:
                out.append(cases[0])
            out.append(c)
    return out


def grp_cases(rnd, G, bounds=ONE_BOUNDS_NEG, prefix="grp"):
    """dbl_body<G>, dadd_body<G> (with the flag) at the bounds g1_28.hip.h states for g1::dbl and g1::dadd; results under
    the bounds carried between calls (X < 10p, Y < 6p, ZZ, ZZZ < 2p, exactly normalized).  Returns the two case lists,
    placed for groups of G lanes."""
    reps = one_reps_for(bounds)
    dbl = []
    for pt in sample_points():
        for which in ("low", "top", "mixed"):
            limbs = reps(pt, rnd, which)

            def chk(out, w=aff_dbl(pt)):
                def lane(flag, regs):
                    assert flag == 0
                    check_point_regs(regs, w, ONE_BOUNDS, strict=True)

                check_group(out, G, lane)

            dbl.append(Case("%s_dbl%d" % (prefix, G), point_words_limbs(limbs), chk, which))
    dadd = []
    for a, b, want, tag in pair_cases(rnd, reps, bounds[1]):
        def chk(out, a=a, want=want, tag=tag):
            def lane(flag, regs):
                if tag.startswith("P+P"):
                    # true exactly for P + P: the caller doubles, so acc must still be the point it was, as it came
                    assert flag == 1, "flag %d for P + P" % flag
                    check_point_regs(regs, affine_of(*[value(l) for l in a]), bounds, strict=True)
                else:
                    assert flag == 0, "flag %d" % flag
                    # a copied operand keeps the bounds it came with; a computed sum is under the carried ones
                    check_point_regs(regs, want, bounds if tag in ("inf+Q", "P+inf") else ONE_BOUNDS, strict=True)

            check_group(out, G, lane)

        dadd.append(Case("%s_dadd%d" % (prefix, G), point_words_limbs(a) + point_words_limbs(b), chk, tag))
    return grp_place(dbl, G), grp_place(dadd, G)


def affine_operand(pt, rnd, negated):
    """(x2, y2) as madd takes them: x canonical, y canonical or, for a subtraction, 2p - y"""
    x, y = to_mont(pt[0]), to_mont(pt[1])
    return limbs_strict(x), limbs_strict(2 * P - y if negated else y)


def madd_cases(rnd, op="grp_madd4", G=4, bounds=ONE_BOUNDS, place=True):
    """acc += (x2, y2) at the bounds of g1::madd (X < 10p, Y < 6p): ordinary, acc at infinity, P + P, P + (-P)"""
    reps = one_reps_for(bounds)
    pts = sample_points()
    cases = []
    for i, p in enumerate(pts):
        q = pts[(i + 5) % len(pts)]
        for which in ("low", "top", "mixed"):
            for tag, acc, operand, neg in (("P+Q", p, q, False), ("P-Q", p, q, True), ("inf+Q", None, q, False), ("inf-Q", None, q, True),
                                           ("P+P", p, p, False), ("P-(-P)", p, aff_neg(p), True), ("P-P", p, p, True), ("P+(-P)", p, aff_neg(p), False)):
                x2, y2 = affine_operand(operand, rnd, neg)
                want = aff_add(acc, aff_neg(operand) if neg else operand)
                a = reps(acc, rnd, which)

                def chk(out, want=want):
                    def lane(flag, regs):
                        # set_affine leaves y2 as it came (< 2p) and ZZ = ZZZ = one()
                        check_point_regs(regs, want, ONE_BOUNDS, strict=True)

                    check_group(out, G, lane)

                cases.append(Case(op, point_words_limbs(a) + x2 + y2, chk, tag + " " + which))
    return grp_place(cases, G) if place else cases


# ---- the boundary between the two contracts: single-lane routines on points the wide code stored (X, Y < 18p) ----
STORED_BOUNDS = (18, 18, 2, 2)  # what g1w::store writes, exactly normalized


def boundary_cases(rnd):
    """The single-lane consumers of arrays the wide kernels store into ("Bounds across the wide / single-lane
    boundary"), fed what their producers may emit at the widest: X, Y just under 18p, exactly normalized.
      one_dadd          g1::dadd(acc, b): b stored by the wide code, acc under the single-lane bounds (k_final's Horner), and
                        acc itself a stored point with b != acc (the first window: acc = b is a copy)
      one_dadd_unequal  the same for g1::dadd_unequal
      one_dbl_k         g1::dbl_k of a stored point (k_final after the copy)
      one_to_blst       g1::to_blst_jacobian of a stored point (k_final, k_g1_store)
      one_reduce_xy     g1::reduce_xy: a stored point back under X, Y < 2p for the routines that negate or double it"""
    stored = one_reps_for(STORED_BOUNDS)
    own = one_reps_for(ONE_BOUNDS)
    pts = sample_points()
    out = {"one_dadd": [], "one_dadd_unequal": [], "one_dbl_k": [], "one_to_blst": [], "one_reduce_xy": []}

    def point_check(want, bounds):
        def chk(o):
            check_group(o, 1, lambda flag, regs: check_point_regs(regs, want, bounds, strict=True))

        return chk

    for i, p in enumerate(pts):
        q = pts[(i + 7) % len(pts)]
        for which in ("top", "mixed"):
            sp, sq = stored(p, rnd, which), stored(q, rnd, "top")
            rows = [  # (acc, b, expected, bounds of the result)
                (own(p, rnd, "top"), sq, aff_add(p, q), ONE_BOUNDS),
                (own(q, rnd, "mixed"), sq, aff_dbl(q), ONE_BOUNDS),                     # P + P: acc under the single-lane bounds is doubled
                (own(q, rnd, "top"), neg_reps(sq, rnd, 18), None, ONE_BOUNDS),
                ([[0] * L] * 4, sq, q, STORED_BOUNDS),                                  # the copy
                (sp, sq, aff_add(p, q), ONE_BOUNDS),                                    # a stored accumulator, b != acc
                (sp, [[0] * L] * 4, p, STORED_BOUNDS),
                (sp, neg_reps(stored(p, rnd, "top"), rnd, 18), None, ONE_BOUNDS),
            ]
            for acc, b, want, bounds in rows:
                words = point_words_limbs(acc) + point_words_limbs(b)
                out["one_dadd"].append(Case("one_dadd", words, point_check(want, bounds)))

                def chk_u(o, want=want, bounds=bounds, acc=acc, same=want is not None and acc != [[0] * L] * 4 and want == aff_dbl(affine_of(*[value(l) for l in acc]))
                          and affine_of(*[value(l) for l in acc]) == affine_of(*[value(l) for l in b])):
                    def lane(flag, regs):
                        assert flag == (1 if same else 0), "flag %d" % flag
                        if same:
                            check_point_regs(regs, affine_of(*[value(l) for l in acc]), ONE_BOUNDS, strict=True)
                        else:
                            check_point_regs(regs, want, bounds, strict=True)

                    check_group(o, 1, lane)

                out["one_dadd_unequal"].append(Case("one_dadd_unequal", words, chk_u))
            for k in (0, 1, 3):
                want = p
                for _ in range(k):
                    want = aff_dbl(want)
                out["one_dbl_k"].append(Case("one_dbl_k", point_words_limbs(sp) + [k], point_check(want, STORED_BOUNDS if k == 0 else ONE_BOUNDS)))

            def chk_blst(o, p=p):
                flag, w = o[0], o[1:37]
                assert flag == 0 and o[37:GRP_OUT] == [SENTINEL] * (GRP_OUT - 37)
                X, Y, Z = (sum(x << (32 * j) for j, x in enumerate(w[12 * c:12 * c + 12])) for c in range(3))
                assert X < P and Y < P and Z < P, "not canonical"
                r384 = pow(1 << 384, -1, P)
                x, y, z = X * r384 % P, Y * r384 % P, Z * r384 % P   # Jacobian (X ZZ, Y ZZZ, ZZ): x = X / Z^2, y = Y / Z^3
                zi = pow(z, -1, P)
                assert (x * zi * zi % P, y * zi * zi * zi % P) == p, "wrong point"

            out["one_to_blst"].append(Case("one_to_blst", point_words_limbs(sp), chk_blst))
            out["one_reduce_xy"].append(Case("one_reduce_xy", point_words_limbs(sp), point_check(p, (2, 2, 2, 2))))
    out["one_dbl_k"].append(Case("one_dbl_k", [0] * PT + [3], point_check(None, ONE_BOUNDS)))
    out["one_to_blst"].append(Case("one_to_blst", [0] * PT, lambda o: (o[:37] == [0] * 37) or (_ for _ in ()).throw(AssertionError("infinity"))))
    out["one_reduce_xy"].append(Case("one_reduce_xy", [0] * PT, point_check(None, ONE_BOUNDS)))
    return out


def single_lane_contract_cases(rnd):
    """g1::madd and g1::chain_add never read a point the wide code stored (their accumulator is the lane's own); they are
    held to their own bounds here, on the device as on the host: madd X < 10p, Y < 6p; chain_add's three chain states"""
    out = {"one_madd": madd_cases(rnd, "one_madd", 1, place=False)}
    own = one_reps_for(ONE_BOUNDS)
    pts = sample_points()
    cases = []
    for i, p in enumerate(pts):
        q = pts[(i + 5) % len(pts)]
        for neg in (False, True):
            m = 0xffffffff if neg else 0
            sq = aff_neg(q) if neg else q
            x2, y2 = limbs_strict(to_mont(q[0])), limbs_strict(to_mont(q[1]))
            rows = [(0, None, sq, 1)]                                  # CHAIN_EMPTY -> CHAIN_AFFINE
            for acc_pt, want_st in ((p, 2), (sq, 2), (aff_neg(sq), 0)):
                # CHAIN_AFFINE: x canonical, y canonical or 2p - y' for the table's y' = p - y: y or p + y
                ay = to_mont(acc_pt[1])
                for yrep in (ay, P + ay):
                    acc = [limbs_strict(to_mont(acc_pt[0])), limbs_strict(yrep), limbs_strict(to_mont(1)), limbs_strict(to_mont(1))]
                    rows.append((1, acc, aff_add(acc_pt, sq), want_st))
                rows.append((2, own(acc_pt, rnd, "top"), aff_add(acc_pt, sq), want_st))     # CHAIN_XYZZ at its bounds
                rows.append((2, own(acc_pt, rnd, "mixed"), aff_add(acc_pt, sq), want_st))
            for st, acc, want, want_st in rows:
                acc = acc or [[0] * L] * 4

                def chk(o, want=want, want_st=want_st):
                    def lane(flag, regs):
                        assert flag == want_st, "chain state %d, expected %d" % (flag, want_st)
                        check_point_regs(regs, want, ONE_BOUNDS, strict=True)

                    check_group(o, 1, lane)

                cases.append(Case("one_chain_add", point_words_limbs(acc) + [st] + x2 + y2 + [m], chk))
    out["one_chain_add"] = cases
    return out


# ------------------------------------------------------------------------------------------------ the whole list
SEED = 20281


def all_cases():
    """op -> cases, in the order they are sent (one block, one kernel launch, per op).  Case 1 of every block is the one
    a -DLANE_CHECK_PLANT_ERROR build spoils."""
    rnd = random.Random(SEED)
    blocks = {}
    blocks["wnorm"] = wnorm_cases(rnd, False)
    blocks["wnorm_full"] = wnorm_cases(rnd, True)
    for c in waddsub_cases(rnd):
        blocks.setdefault(c.op, []).append(c)
    blocks["wmul4"] = wmul_cases(rnd)
    blocks["wsqr"] = wsqr_cases(rnd)
    blocks["wdbl"] = wdbl_cases(rnd)
    blocks["wide_roundtrip"] = roundtrip_cases(rnd)
    blocks["is_zero"] = is_zero_cases(rnd)
    blocks["load_store"] = load_store_cases(rnd)
    blocks["dbl"] = dbl_cases(rnd)
    blocks["dadd"] = dadd_cases(rnd)
    blocks["dbl_k"] = dbl_k_cases(rnd)
    blocks["add_n"] = add_n_cases(rnd)
    blocks["chain"] = chain_cases(rnd)
    for G in (1, 2, 4):
        blocks["grp_dbl%d" % G], blocks["grp_dadd%d" % G] = grp_cases(rnd, G)
    blocks["grp_madd4"] = madd_cases(rnd)
    blocks.update(boundary_cases(rnd))
    blocks.update(single_lane_contract_cases(rnd))
    for op, cases in blocks.items():
        nin = OPS[op][0]
        assert len(cases) >= 2, op
        for c in cases:
            assert c.op == op and len(c.words) == nin and all(0 <= w < 1 << 32 for w in c.words), (op, len(c.words), nin)
    return blocks


def encode(blocks):
    """the text the harness (or the host checker) reads"""
    parts = []
    for op, cases in blocks.items():
        parts.append("%s %d\n" % (op, len(cases)))
        parts += [" ".join("%x" % w for w in c.words) + "\n" for c in cases]
    return "".join(parts)


def decode(text, blocks):
    """what the harness printed -> op -> list of word lists; raises on anything but the expected shape"""
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
    """[(op, case index, message)] for every case whose checker objects"""
    bad = []
    for op, cases in blocks.items():
        for i, (c, o) in enumerate(zip(cases, outs[op])):
            try:
                c.check(o)
            except AssertionError as e:
                bad.append((op, i, "%s%s" % (c.tag + ": " if c.tag else "", e)))
    return bad
