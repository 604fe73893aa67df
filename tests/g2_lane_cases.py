"""The cases and the checkers of tests/device_checks/g2_check.hip, on Python integers only: fp28.hip.h's primitives,
Fp2 and the twist points of g2_28.hip.h, the wire format and membership of g2_io.hip.h, the term and the tree of
g2_lincomb.hip.h, each at the bounds its header states.  The reference is the plain integer model — Fp2 as pairs mod p,
the chord / tangent law on affine points, tests/codec_model.py for the wire format and psi — never another build of the
code under test.  tests/test_g2_arith_gpu.py runs the cases on the device, tests/test_g2_device_cases_cpu.py on the
harness's host form.

A block is a list of cases of one op that run in ONE kernel launch, case i in lane i % 64 of workgroup i / 64.  Blocks
are named "<op>" or "<op>/<flavour>"; the point ops and `term` come twice:
  mixed    every wave holds every exceptional kind next to generic cases (mix() deals them out and asserts it);
  uniform  whole waves of one exceptional kind (64 x P + P, 64 x P - P, 64 x infinity + P, 64 flagged entries, 64 zero
           scalars ...): a wave-uniform branch is other generated code than a divergent one.
Every generator asserts the routine's precondition before it emits a case; every checker verifies the normalisation of
the output, its value bound from the header's table, and its residue or group element."""
import random

import codec_model as CM
import g2_encodings as G2E
import setup_model as S
from test_g2_lane_cpu import DONE, DOUBLE, INF, LOW_ONES, M28, P, R392, aff_add, f2add, f2inv, f2mul, f2sub, pattern_values, rep, twist_point, value

SEED = 0x6232
RINV = pow(R392, -1, P)
R_FR = S.R
FE, F2W, JAC, AFF = 14, 28, 84, 56
LAZY_LIMB = (1 << 28) + (1 << 29)  # what sub_lazy leaves: limbs below this

# op -> (words in, words out), as g2_check.hip's table
OPS = {"fp_mul": (28, 14), "fp_sqr": (14, 14), "fp_mul2": (56, 14), "fp_ssl8": (29, 14), "fp_ssl16": (29, 14),
       "fp_sub2bc": (42, 14), "fp_norm": (14, 14), "fp_iszero": (14, 1), "fp_canon": (14, 14), "fp_from_blst": (12, 14),
       "fp_to_blst": (14, 12), "fp_pack": (14, 12), "fp_unpack": (12, 14),
       "f2_add": (56, 28), "f2_dbl": (28, 28), "f2_sub4": (56, 28), "f2_sub8": (56, 28), "f2_sub16": (56, 28),
       "f2_sub32": (56, 28), "f2_neg2": (28, 28), "f2_neg16": (28, 28), "f2_mul": (56, 28), "f2_sqr": (28, 28),
       "f2_mulfe": (42, 28), "f2_red": (28, 28), "f2_inv": (28, 28), "f2_iszero": (28, 1),
       "g2_dbl": (84, 84), "g2_madd": (140, 85), "g2_maddc": (140, 84), "g2_maddtab": (142, 84), "g2_add": (168, 84),
       "g2_fedback": (224, 15 * 84), "g2_toaff": (84, 57), "g2_fromblst": (72, 84), "g2_toblst": (84, 72),
       "io_canon2": (14, 14), "io_lex": (28, 1), "io_sqrt": (28, 29), "io_uncompress": (96, 58), "io_compress": (84, 96),
       "io_psi": (56, 56), "io_ing2": (57, 1), "io_psiconst": (1, 56),
       "lc_term": (80, 84), "lc_tree1": (64 * 84, 32 * 84), "lc_tree6": (64 * 84, 84)}
for _k in (2, 4, 8, 16, 32):
    OPS["fp_sub%d" % _k] = OPS["fp_subl%d" % _k] = (28, 14)
    OPS["fp_neg%d" % _k] = (14, 14)

FP_OPS = tuple(op for op in OPS if op.startswith("fp_"))
F2_OPS = tuple(op for op in OPS if op.startswith("f2_"))
POINT_OPS = ("g2_dbl", "g2_madd", "g2_maddc", "g2_maddtab", "g2_add")  # emitted mixed and uniform
G2_PLAIN_OPS = ("g2_fedback", "g2_toaff", "g2_fromblst", "g2_toblst")
IO_OPS = tuple(op for op in OPS if op.startswith("io_"))
LAYERS = {
    "fp": FP_OPS, "fp2": F2_OPS,
    "g2_mixed": tuple(op + "/mixed" for op in POINT_OPS) + G2_PLAIN_OPS, "g2_uniform": tuple(op + "/uniform" for op in POINT_OPS),
    "g2io": IO_OPS, "g2lc_mixed": ("lc_term/mixed", "lc_tree1", "lc_tree6"), "g2lc_uniform": ("lc_term/uniform",),
}


class Case:
    __slots__ = ("op", "words", "check", "tag", "kind")

    def __init__(self, op, words, check, tag="", kind="generic"):
        self.op, self.words, self.check, self.tag, self.kind = op, words, check, tag, kind


def op_of(block):
    return block.split("/")[0]


# ------------------------------------------------------------------------------------------------ limbs
def nl(v):
    """the normalized representation: limbs 0..12 below 2^28, the rest in the top limb"""
    assert 0 <= v < 1 << 396
    return [(v >> (28 * i)) & M28 for i in range(13)] + [v >> 364]


def w32(v, n):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def normalized(l):
    return all(0 <= x <= M28 for x in l[:13]) and 0 <= l[13] < 1 << 32


def need(cond, msg):
    if not cond:
        raise AssertionError(msg)


def check_fe(l, bound, residue=None, exact=None, what="result", inclusive=False, congruent=None):
    """normalized, value below bound * p (or at most, for neg<K>), and the value itself, the value mod p, or the field
    element it stands for in Montgomery form"""
    need(len(l) == 14 and normalized(l), "%s not normalized" % what)
    v = value(l)
    need(v < bound * P or (inclusive and v == bound * P), "%s: %d p and more, bound %d p" % (what, v // P, bound))
    if exact is not None:
        need(v == exact, "%s: wrong value" % what)
    if congruent is not None:
        need(v % P == congruent % P, "%s: wrong residue" % what)
    if residue is not None:
        need(v * RINV % P == residue % P, "%s: wrong residue" % what)


def edge_values(k, rnd, nrandom=6):
    """values in [0, k p): multiples of p and their neighbours, an empty top limb, the maximum, the limb patterns"""
    out = [0, 1, k * P - 1, (1 << 364) - 1, 1 << 364, M28]
    for j in range(k):
        out += [j * P, j * P + 1, max(0, j * P - 1)]
    out += pattern_values(k)
    out += [rnd.randrange(k * P) for _ in range(nrandom)]
    return [v for v in out if v < k * P]


def lazy(rnd, bits, top_bits=None):
    """a representation with limbs up to `bits` wide, every fifth at its maximum"""
    l = [rnd.randrange(1 << bits) if rnd.random() < 0.8 else (1 << bits) - 1 for _ in range(14)]
    if top_bits is not None:
        l[13] = rnd.randrange(1 << top_bits)
    return l


# ------------------------------------------------------------------------------------------------ fp28
def mont_check(prod):
    return lambda out: check_fe(out, 2, congruent=prod * RINV)


def fp_product_cases(rnd):
    mul, sqr, mul2 = [], [], []

    def put_mul(a, b, tag):
        assert all(x < 1 << 30 for x in a + b) and value(a) * value(b) < P << 392, tag
        mul.append(Case("fp_mul", a + b, mont_check(value(a) * value(b)), tag))

    def put_sqr(a, tag):
        assert all(x < 1 << 30 for x in a) and value(a) ** 2 < P << 392, tag
        sqr.append(Case("fp_sqr", a, mont_check(value(a) ** 2), tag))

    for ka, kb in ((2, 2), (10, 6), (16, 4), (32, 2), (63, 40), (8, 8), (25, 25), (2520, 1)):
        ra, rb = rnd.randrange(P), rnd.randrange(P)
        put_mul(nl(rep(ra, ka - 1)), nl(rep(rb, kb - 1)), "top of %d x %d" % (ka, kb))
        put_mul(nl(ka * P - 1), nl(kb * P - 1), "the largest values of %d x %d" % (ka, kb))
        for va in pattern_values(ka):
            put_mul(nl(va), nl(pattern_values(kb)[0]), "limb pattern")
        for j in {1, ka // 2, ka - 1}:
            for d in (-1, 0, 1):
                put_mul(nl(j * P + d), nl(rb), "k p and its neighbours")
        put_mul(nl((1 << 364) - 1), nl(rep(rb, kb - 1)), "empty top limb")
    for k in (2, 4, 15, 18, 30, 50):  # 50 p squared is 2500 p^2 <= 2520 p^2
        put_sqr(nl(rep(rnd.randrange(P), k - 1)), "top of %d" % k)
        put_sqr(nl(k * P - 1), "the largest value below %d p" % k)
        for v in pattern_values(k):
            put_sqr(nl(v), "limb pattern")
        for d in (-1, 0, 1):
            put_sqr(nl((k - 1) * P + d), "k p and its neighbours")
    put_sqr(nl((1 << 364) - 1), "empty top limb")
    put_sqr(nl(0), "zero")
    for _ in range(40):  # 30-bit limbs: the value reaches 2^394, the other operand keeps the product below 2^392 p
        a = lazy(rnd, 30)
        bmax = (P << 392) // max(value(a), 1) - 1
        put_mul(a, nl(rnd.randrange(min(bmax, 2 * P))), "30-bit limbs")
        s = lazy(rnd, 29, top_bits=22)
        put_sqr(s, "29-bit limbs")
    put_mul([(1 << 30) - 1] * 13 + [0], nl(P - 1), "every limb 2^30 - 1 under an empty top limb")
    for _ in range(30):  # both operands lazy: the value bound leaves room for that in the low half only
        put_mul(lazy(rnd, 30)[:7] + [0] * 7, lazy(rnd, 30)[:7] + [0] * 7, "both lazy in the low half")
    put_mul([(1 << 30) - 1] * 7 + [0] * 7, [(1 << 30) - 1] * 7 + [0] * 7, "both lazy, every limb at its maximum")
    put_sqr([(1 << 30) - 1] * 7 + [0] * 7, "lazy low half squared")

    def put_mul2(a, b, c, d, tag):
        tot = value(a) * value(b) + value(c) * value(d)
        assert normalized(a) and normalized(c) and all(x < LAZY_LIMB for x in b[:13] + d[:13]) and tot < P << 392, tag
        col = max(sum(a[i] * b[k - i] + c[i] * d[k - i] for i in range(14) if 0 <= k - i < 14) for k in range(27))
        assert col + 14 * (1 << 56) < 1 << 63, tag  # the column bound mul2_inline states
        mul2.append(Case("fp_mul2", a + b + c + d, mont_check(tot), tag))

    ev2 = edge_values(2, rnd)
    top_lazy = 0x1a0110 + 0x1a011 * 8
    for i in range(80):
        a, c = nl(ev2[i % len(ev2)]), nl(rnd.choice(ev2))
        b = [rnd.randrange(LAZY_LIMB) for _ in range(13)] + [rnd.randrange(top_lazy)]
        d = [rnd.randrange(LAZY_LIMB) for _ in range(13)] + [rnd.randrange(top_lazy)]
        put_mul2(a, b, c, d, "one lazy operand per product")
    ones = nl((0x34021 << 364) | LOW_ONES)
    assert value(ones) < 2 * P
    mx = [LAZY_LIMB - 1] * 13 + [top_lazy - 1]
    put_mul2(ones, mx, ones, mx, "every limb at its maximum: the columns at their bound")
    put_mul2(nl(0), mx, ones, mx, "one product zero")
    return {"fp_mul": mul, "fp_sqr": sqr, "fp_mul2": mul2}


def fp_sub_cases(rnd):
    blocks = {}
    for k in (2, 4, 8, 16, 32):
        sub, subl, neg = [], [], []
        for bv in edge_values(k - 1, rnd, 50 if k <= 8 else 12):
            assert bv < (k - 1) * P
            for av in (0, rnd.choice(edge_values(2, rnd)), rnd.choice(edge_values(31, rnd))):
                want = av + k * P - bv
                sub.append(Case("fp_sub%d" % k, nl(av) + nl(bv), lambda o, w=want: check_fe(o, 64, exact=w)))

                def chk_lazy(o, w=want):
                    need(all(x < LAZY_LIMB for x in o[:13]) and o[13] < 1 << 31, "lazy limb bound")
                    need(value(o) == w, "wrong value")
                subl.append(Case("fp_subl%d" % k, nl(av) + nl(bv), chk_lazy))
            neg.append(Case("fp_neg%d" % k, nl(bv), lambda o, w=k * P - bv, k=k: check_fe(o, k, exact=w, inclusive=True)))
        blocks["fp_sub%d" % k], blocks["fp_subl%d" % k], blocks["fp_neg%d" % k] = sub, subl, neg
    # sub_signed_lazy: K = 16 with s < 2p, y < 6p; K = 8 with s < p, y <= 2p
    for k, sb, yvals in ((16, 2, None), (8, 1, None)):
        out = []
        svals = edge_values(sb, rnd, 3)
        yvals = edge_values(6, rnd, 3) if k == 16 else edge_values(2, rnd, 3) + [2 * P]
        pairs = [(sb * P - 1, yvals[2] if k == 16 else 2 * P), (sb * P - 1, 0), (0, max(yvals)), (0, 0)]
        pairs += [(rnd.choice(svals), y) for y in yvals] + [(s, rnd.choice(yvals)) for s in svals]
        assert (sb * P - 1, max(yvals)) in pairs + [(sb * P - 1, max(yvals))]
        pairs.append((sb * P - 1, max(yvals)))  # s and y at their maxima
        for s, y in pairs:
            assert s < sb * P and (y < 6 * P if k == 16 else y <= 2 * P)
            for m in (0, 0xFFFFFFFF):
                want = k * P - y + (s if m == 0 else -s)

                def chk(o, w=want, k=k):
                    need(all(x <= (1 << 30) - 2 for x in o[:13]), "a limb beyond 2^30 - 2 (or wrapped)")
                    need(o[13] < 1 << 21, "top limb negative or beyond 2^21")
                    need(value(o) == w, "wrong value")
                    need((8 * P < w < 18 * P) if k == 16 else (5 * P < w < 9 * P), "value outside the stated interval")
                out.append(Case("fp_ssl%d" % k, nl(s) + nl(y) + [m], chk, "s = %x.., y = %x.., mask %x" % (s >> 350, y >> 350, m)))
        blocks["fp_ssl%d" % k] = out
    out = []
    ev2 = edge_values(2, rnd)
    for i, av in enumerate(edge_values(31, rnd)):
        for b, c in ((ev2[i % len(ev2)], rnd.choice(ev2)), (2 * P - 1, 2 * P - 1), (0, 0)):
            assert b < 2 * P and c < 2 * P
            out.append(Case("fp_sub2bc", nl(av) + nl(b) + nl(c), lambda o, w=av + 8 * P - 2 * b - c: check_fe(o, 64, exact=w)))
    blocks["fp_sub2bc"] = out
    return blocks


def fp_misc_cases(rnd):
    blocks = {}
    out = []
    for i in range(80):  # norm: limbs up to 2^31 under a small top limb; every limb at its maximum: the longest ripple
        l = [(1 << 31) - 1] * 13 + [5] if i == 0 else [M28] * 13 + [0] if i == 2 else lazy(rnd, (29, 30, 31)[i % 3], top_bits=22)
        assert all(x < 1 << 31 for x in l)

        def chk(o, w=value(l)):
            need(normalized(o), "not normalized")
            need(value(o) == w, "value changed")
        out.append(Case("fp_norm", l, chk))
    blocks["fp_norm"] = out
    # the exact zero test: normalized or lazy, value < 64 p
    out = []
    zc = lambda l, want, tag: out.append(Case("fp_iszero", l, lambda o, w=want: need(o == [w], "verdict %s, expected %d" % (o, w)), tag))
    for j in range(64):
        zc(nl(j * P), 1, "%d p" % j)
        for d in (1, 1 << 200, 1 << 364):
            if j * P + d < 64 * P:
                zc(nl(j * P + d), 0, "%d p + %x" % (j, d))
    for _ in range(32):  # a lazy multiple: the limb-wise sum of two normalized multiples
        x, y = rnd.randrange(1, 32), rnd.randrange(1, 32)
        zc([a + b for a, b in zip(nl(x * P), nl(y * P))], 1, "lazy %d p + %d p" % (x, y))
    fp_class = 0
    for j in range(64):  # what passes the filter without being a multiple: limb 0 of j p under other limbs
        for _ in range(2):
            v = (rnd.randrange(1, 63 * P >> 28) << 28) | (j * P & M28)
            if v % P and v < 64 * P:
                assert (v & M28) * 0x0030003 & M28 < 64
                zc(nl(v), 0, "passes the filter as %d p" % j)
                fp_class += 1
    assert fp_class >= 64
    for _ in range(40):
        v = rnd.randrange(64 * P)
        zc(nl(v), int(v % P == 0), "random")
    blocks["fp_iszero"] = out
    out = []
    for v in [0, 1, P - 1, P, P + 1, 2 * P - 1, (1 << 364) - 1, 1 << 364] + pattern_values(2) + [rnd.randrange(2 * P) for _ in range(56)]:
        assert v < 2 * P
        out.append(Case("fp_canon", nl(v), lambda o, w=v % P: check_fe(o, 1, exact=w), "%x.." % (v >> 350)))
    blocks["fp_canon"] = out
    # the blst conversions: from_blst x 2^384 -> x 2^392, to_blst back (canonical), pack / unpack bit re-slicing
    fb, tb, pk, up = [], [], [], []
    vals = [0, 1, P - 1, P - 2, (1 << 380), (1 << 381) - 1, (1 << 384) - 1, P, P + 1] + [rnd.randrange(P) for _ in range(60)]
    for v in vals:
        assert v < 1 << 384
        fb.append(Case("fp_from_blst", w32(v, 12), lambda o, v=v: check_fe(o, 2, congruent=v << 8)))
        up.append(Case("fp_unpack", w32(v, 12), lambda o, v=v: (need(o[13] < 1 << 20, "top limb"), check_fe(o, 64, exact=v))))
        pk.append(Case("fp_pack", nl(v), lambda o, v=v: need(o == w32(v, 12), "pack: wrong words")))
    for i in range(72):
        k = (1, 2, 63, 64, 2520)[i % 5]
        v = [rep(rnd.randrange(P), k - 1), k * P - 1, (k - 1) * P][i % 3] if i < 60 else pattern_values(64)[i % 6]
        assert v < 2520 * P and all(x < 1 << 30 for x in nl(v))
        tb.append(Case("fp_to_blst", nl(v), lambda o, v=v: need(o == w32(v * pow(256, -1, P) % P, 12), "to_blst: not the canonical residue")))
    blocks.update({"fp_from_blst": fb, "fp_to_blst": tb, "fp_pack": pk, "fp_unpack": up})
    return blocks


# ------------------------------------------------------------------------------------------------ Fp2
def res2(a):
    """the field element a pair of representatives stands for"""
    return (a[0] * RINV % P, a[1] * RINV % P)


def f2words(a):
    return nl(a[0]) + nl(a[1])


def check_f2(o, bounds, want=None, exact=None, what="result", inclusive=False):
    for c in (0, 1):
        check_fe(o[14 * c:14 * c + 14], bounds[c], residue=None if want is None else want[c], exact=None if exact is None else exact[c],
                 what="%s c%d" % (what, c), inclusive=inclusive)


# (name, bound of a, bound of b, output bounds): the table of tests/test_g2_lane_cpu.py, from g2_28.hip.h
F2_TABLE = [("add", 32, 31, (63, 63)), ("dbl", 31, 1, (62, 62)), ("sub4", 10, 3, (14, 14)), ("sub8", 10, 7, (18, 18)),
            ("sub16", 10, 15, (26, 26)), ("sub32", 16, 31, (48, 48)), ("neg2", 1, 1, (2, 2)), ("neg16", 15, 1, (16, 16)),
            ("mul", 21, 30, (6, 10)), ("mul", 63, 10, (6, 10)), ("mul", 25, 25, (6, 10)), ("sqr", 15, 1, (2, 4)),
            ("mulfe", 63, 40, (2, 2)), ("red", 63, 1, (2, 2)), ("inv", 15, 1, (2, 2))]
F2_UNARY = ("dbl", "neg2", "neg16", "sqr", "red", "inv")


def f2_model(name, a, b):
    """(exact values or None, residues) of the routine on representatives a, b"""
    ra, rb = res2(a), res2(b)
    if name == "add":
        return (a[0] + b[0], a[1] + b[1]), f2add(ra, rb)
    if name == "dbl":
        return (2 * a[0], 2 * a[1]), f2add(ra, ra)
    if name.startswith("sub"):
        k = int(name[3:])
        return (a[0] + k * P - b[0], a[1] + k * P - b[1]), f2sub(ra, rb)
    if name.startswith("neg"):
        k = int(name[3:])
        return (k * P - a[0], k * P - a[1]), f2sub((0, 0), ra)
    if name == "mul":
        return None, f2mul(ra, rb)
    if name == "sqr":
        return None, f2mul(ra, ra)
    if name == "mulfe":
        return None, (ra[0] * rb[0] % P, ra[1] * rb[0] % P)
    if name == "red":
        return None, ra
    if name == "inv":
        return None, f2inv(ra)
    raise KeyError(name)


def f2_cases(rnd):
    blocks = {}
    for name, ba, bb, ob in F2_TABLE:
        out = blocks.setdefault("f2_" + name, [])
        rv = lambda bound: rep(rnd.randrange(P), rnd.randrange(bound))
        top = lambda bound: rep(rnd.randrange(P), bound - 1)
        pairs = []
        for it in range(24):
            pick = (top, rv)[it & 1]  # case 0 and 1 of a block at the top of the bound
            pairs.append(((pick(ba), pick(ba)), (pick(bb), pick(bb)), "top" if pick is top else "random"))
        pa, pb = pattern_values(ba), pattern_values(bb)
        for va in pa:
            for vb in pb[:3]:
                pairs.append(((va, pa[0]), (vb, pb[-1]), "limb pattern"))
                pairs.append(((pa[-1], va), (pb[0], vb), "limb pattern"))
        for j in (1, ba - 1):
            for d in (-1, 0, 1):
                if 0 <= j * P + d < ba * P:
                    pairs.append(((j * P + d, top(ba)), (top(bb), max(0, (bb - 1) * P + d)), "k p and its neighbours"))
        pairs.append((((1 << 364) - 1, ba * P - 1), (bb * P - 1, (1 << 364) - 1), "empty top limb, largest value"))
        for a, b, tag in pairs:
            assert all(0 <= c < ba * P for c in a) and all(0 <= c < bb * P for c in b), name  # the table's precondition
            if name == "inv" and res2(a) == (0, 0):
                continue
            exact, want = f2_model(name, a, b)
            words = f2words(a) + ([] if name in F2_UNARY else nl(b[0]) if name == "mulfe" else f2words(b))
            out.append(Case("f2_" + name, words, lambda o, ob=ob, want=want, exact=exact, inc=name.startswith("neg"):
                            check_f2(o, ob, want, exact, inclusive=inc), "%s (a < %d, b < %d)" % (tag, ba, bb)))
    out = []
    zc = lambda a, want, tag: out.append(Case("f2_iszero", f2words(a), lambda o, w=want: need(o == [w], "verdict %s, expected %d" % (o, w)), tag))
    for k0 in (0, 1, 13, 62, 63):
        for k1 in (0, 5, 62, 63):
            zc((k0 * P, k1 * P), 1, "%d p, %d p" % (k0, k1))
            zc((k0 * P + 1, k1 * P), 0, "c0 one off")
            zc((k0 * P, k1 * P + (1 << 364) if k1 < 63 else k1 * P + 1), 0, "c1 one off")
    for _ in range(24):
        a = (rep(rnd.randrange(P), 62), rep(rnd.randrange(P), 62))
        zc(a, int(res2(a) == (0, 0)), "random at the top")
    blocks["f2_iszero"] = out
    return blocks


# ------------------------------------------------------------------------------------------------ points
def neg_pt(a):
    return None if a is None else (a[0], f2sub((0, 0), a[1]))


def jac(aff, z, ks):
    """representatives of the Jacobian point over aff with this Z plus ks multiples of p (six); None: all-zero"""
    if aff is None:
        return [0] * 6
    z2 = f2mul(z, z)
    x, y = f2mul(aff[0], z2), f2mul(aff[1], f2mul(z2, z))
    return [rep(c, k) for c, k in zip(x + y + z, ks)]


def jwords(comps):
    return [w for c in comps for w in nl(c)]


def affine_of(comps):
    """the affine point (field elements) six normalized limb lists stand for; None when Z is all-zero"""
    if all(x == 0 for c in comps[4:6] for x in c):
        return None
    v = [value(c) * RINV % P for c in comps]
    zi = f2inv((v[4], v[5]))
    zi2 = f2mul(zi, zi)
    return f2mul((v[0], v[1]), zi2), f2mul((v[2], v[3]), f2mul(zi2, zi))


def check_point(o, bounds, want, what="point"):
    need(len(o) == 84, "%s: %d words" % (what, len(o)))
    comps = [o[14 * k:14 * k + 14] for k in range(6)]
    for c, b in zip(comps, bounds):
        need(normalized(c), "%s not normalized" % what)
        need(value(c) < b * P, "%s: %d p and more, bound %d p" % (what, value(c) // P, b))
    got = affine_of(comps)
    if got is None:
        need(all(x == 0 for x in o), "%s: the identity is not all-zero" % what)
    need((got is None) == (want is None), "%s: %s, expected %s" % (what, "infinity" if got is None else "a finite point", "infinity" if want is None else "a finite point"))
    need(got == want, "%s: not the group law's answer" % what)


B_DBL, B_MADD, B_ADD = (2, 2, 2, 2, 10, 10), (3, 3, 3, 3, 10, 10), (2, 2, 2, 2, 10, 10)
TOP_MADD, TOP_DBL, TOP_AFF = [2, 2, 2, 2, 9, 9], [14, 14, 14, 14, 20, 20], [14] * 6


class Pool:
    """curve points of the twist, found once: random ones, the order-13 point and its multiples, generator multiples"""

    def __init__(self, rnd, n=12):
        self.rnd = rnd
        self.pts = [twist_point(rnd) for _ in range(n)]
        self.t = CM.torsion_point(13)
        self.tm = [None]
        for _ in range(13):
            self.tm.append(aff_add(self.tm[-1], self.t))
        assert self.tm[13] is None and self.tm[12] == neg_pt(self.t)
        self.g = [CM.G2, CM.mul(7, CM.G2), CM.mul(12, CM.G2)]

    def pt(self, i=None):
        return self.pts[self.rnd.randrange(len(self.pts)) if i is None else i % len(self.pts)]

    def z(self):
        return (self.rnd.randrange(P), self.rnd.randrange(P))

    def ks(self, top, hi):
        return list(top) if hi else [self.rnd.randrange(k + 1) for k in top]


def mix(cases, rnd):
    """deal the cases into waves of 64 (the last one partial) so that every wave holds every kind, shuffle inside each
    wave, assert the mix"""
    kinds = sorted({c.kind for c in cases})
    assert "generic" in kinds
    n = len(cases)
    nw = (n + 63) // 64
    cap = [min(64, n - 64 * w) for w in range(nw)]
    assert cap[-1] >= len(kinds), "the partial wave has %d lanes for %d kinds" % (cap[-1], len(kinds))
    left = {k: [c for c in cases if c.kind == k] for k in kinds}
    waves = [[left[k].pop() for k in kinds] for _ in range(nw)]  # one of every kind first
    rest = [c for k in kinds for c in left[k]]
    rnd.shuffle(rest)
    for w in range(nw):
        while len(waves[w]) < cap[w]:
            waves[w].append(rest.pop())
    assert not rest
    out = []
    for w, wave in enumerate(waves):
        assert len(wave) == cap[w]
        assert {c.kind for c in wave} == set(kinds), ("wave %d lacks" % w, set(kinds) - {c.kind for c in wave})
        rnd.shuffle(wave)
        out += wave
    return out


def uniform(per_kind):
    """whole waves of one kind each"""
    out = []
    for kind, cases in per_kind:
        assert len(cases) % 64 == 0 and len(cases) >= 64 and all(c.kind == kind for c in cases), kind
        out += cases
    for w in range(len(out) // 64):
        assert len({c.kind for c in out[64 * w:64 * w + 64]}) == 1
    return out


def madd_case(op, pool, kind, hi, rnd):
    """one case of g2_madd / g2_maddc: (P, affine Q) of this kind; P at the top of X1, Y1 < 3, Z1 < 10 when hi"""
    a, b, z = pool.pt(), pool.pt(), pool.z()
    ks = pool.ks(TOP_MADD, hi)
    kp = [2] * 4 if hi else [rnd.randrange(3) for _ in range(4)]
    while a[0] == b[0]:
        b = pool.pt()
    if kind == "generic":
        p, q, state, want = jac(a, z, ks), b, DONE, aff_add(a, b)
    elif kind == "P + P":
        p, q, state, want = jac(b, z, ks), b, DOUBLE, aff_add(b, b)
    elif kind == "P - P":
        p, q, state, want = jac(b, z, ks), neg_pt(b), INF, None
    elif kind == "infinity + P":
        p, q, state, want = [0] * 6, b, DONE, b
    elif kind == "equal x, other y":
        q = (b[0], f2add(b[1], (1 + rnd.randrange(9), rnd.randrange(9))))
        p, state, want = jac(b, z, ks), INF, None
    elif kind == "Z = 1":
        p, q, state, want = jac(a, (1, 0), [0] * 6), b, DONE, aff_add(a, b)
    elif kind == "order 13":
        i = 1 + rnd.randrange(11)
        p, q, state, want = jac(pool.tm[i], z, ks), pool.tm[13 - i], INF, None
    else:
        raise KeyError(kind)
    qr = [rep(c, k) for c, k in zip(q[0] + q[1], kp)]
    assert all(c < 3 * P for c in p[:4] + qr) and all(c < 10 * P for c in p[4:])  # madd's row of the table
    words = jwords(p) + [w for c in qr for w in nl(c)]
    if op == "g2_madd":
        def chk(o, p=p, state=state, want=want, q=q):
            need(o[0] == state, "state %d, expected %d" % (o[0], state))
            if state == DOUBLE:
                need(o[1:] == jwords(p), "MADD_DOUBLE must leave P alone")
            elif p == [0] * 6:
                need(o[1:] == jwords([rep(c, k) for c, k in zip(q[0] + q[1], kp)] + [rep(1, 0), 0]), "infinity + P is P with Z = one")
            else:
                check_point(o[1:], B_MADD, want)
    else:
        def chk(o, want=want, dbl=kind == "P + P"):
            check_point(o, B_DBL if dbl else B_MADD, want)
    return Case(op, words, chk, kind + (" at the top" if hi else ""), kind)


MADD_KINDS = ("generic", "P + P", "P - P", "infinity + P", "equal x, other y", "Z = 1", "order 13")


def madd_blocks(pool, rnd):
    blocks = {}
    for op in ("g2_madd", "g2_maddc"):
        cases = [madd_case(op, pool, kind, i & 1, rnd) for kind in MADD_KINDS for i in range(12 if kind != "generic" else 88)]
        blocks[op + "/mixed"] = mix(cases, rnd)
        blocks[op + "/uniform"] = uniform([(k, [madd_case(op, pool, k, i & 1, rnd) for i in range(64)]) for k in ("P + P", "P - P", "infinity + P")])
    return blocks


TAB_KINDS = ("generic", "minus", "flagged", "flagged onto infinity", "infinity minus P", "infinity plus P", "P + P", "P - P", "-P - P")


def tab_case(pool, kind, hi, rnd):
    a, b, z = pool.pt(), pool.pt(), pool.z()
    while a[0] == b[0]:
        b = pool.pt()
    ks = pool.ks(TOP_MADD, hi)
    nb = neg_pt(b)
    flags, neg = 0, 0
    if kind == "generic":
        p, want = jac(a, z, ks), aff_add(a, b)
    elif kind == "minus":
        p, neg, want = jac(a, z, ks), 1, aff_add(a, nb)
    elif kind == "flagged":
        p, flags, neg, want = jac(a, z, ks), 1, hi, a
    elif kind == "flagged onto infinity":
        p, flags, neg, want = [0] * 6, 1, hi, None
    elif kind == "infinity minus P":
        p, neg, want = [0] * 6, 1, nb
    elif kind == "infinity plus P":
        p, want = [0] * 6, b
    elif kind == "P + P":
        p, want = jac(b, z, ks), aff_add(b, b)
    elif kind == "P - P":
        p, neg, want = jac(b, z, ks), 1, None
    elif kind == "-P - P":
        p, neg, want = jac(nb, z, ks), 1, aff_add(nb, nb)
    else:
        raise KeyError(kind)
    e = [rep(c, 0) for c in b[0] + b[1]]
    assert all(c < P for c in e) and all(c < 3 * P for c in p[:4]) and all(c < 10 * P for c in p[4:])  # canonical entry, P as madd
    words = jwords(p) + [w for c in e for w in nl(c)] + [flags, 0xFFFFFFFF if neg else 0]

    def chk(o, p=p, flags=flags, want=want):
        if flags:
            need(o == jwords(p), "a flagged entry must leave P alone")
        check_point(o, B_MADD, want)
    return Case("g2_maddtab", words, chk, kind + (" at the top" if hi else ""), kind)


def tab_blocks(pool, rnd):
    cases = [tab_case(pool, kind, i & 1, rnd) for kind in TAB_KINDS for i in range(10 if kind != "generic" else 80)]
    return {"g2_maddtab/mixed": mix(cases, rnd),
            "g2_maddtab/uniform": uniform([(k, [tab_case(pool, k, i & 1, rnd) for i in range(64)]) for k in ("flagged", "P + P", "P - P", "infinity minus P")])}


ADD_KINDS = ("generic", "P + P", "P - P", "infinity + Q", "P + infinity", "infinity + infinity", "Z = 1", "P + P, Z = 1", "order 13: T + T",
             "order 13: T + 12 T", "order 13: 6 T + 7 T")


def add_case(pool, kind, hi, rnd):
    a, b = pool.pt(), pool.pt()
    while a[0] == b[0]:
        b = pool.pt()
    ks = lambda: pool.ks(TOP_MADD, hi)
    one = (1, 0)
    same = None  # the operand that must come back as it is
    if kind == "generic":
        p, q, want = jac(a, pool.z(), ks()), jac(b, pool.z(), ks()), aff_add(a, b)
    elif kind == "P + P":  # the same point under two different Z
        p, q, want = jac(a, pool.z(), ks()), jac(a, pool.z(), ks()), aff_add(a, a)
    elif kind == "P - P":
        p, q, want = jac(a, pool.z(), ks()), jac(neg_pt(a), pool.z(), ks()), None
    elif kind == "infinity + Q":
        p, q, want = [0] * 6, jac(b, pool.z(), ks()), b
        same = q
    elif kind == "P + infinity":
        p, q, want = jac(a, pool.z(), ks()), [0] * 6, a
        same = p
    elif kind == "infinity + infinity":
        p, q, want = [0] * 6, [0] * 6, None
    elif kind == "Z = 1":
        zs = [(one, [0] * 6), (pool.z(), ks())]
        (z1, k1), (z2, k2) = zs if hi else zs[::-1]
        if rnd.random() < 0.3:
            z1, k1, z2, k2 = one, [0] * 6, one, [0] * 6
        p, q, want = jac(a, z1, k1), jac(b, z2, k2), aff_add(a, b)
    elif kind == "P + P, Z = 1":
        p, q, want = jac(a, one, [0] * 6), jac(a, one, [0] * 6), aff_add(a, a)
    elif kind.startswith("order 13"):
        i, j = {"order 13: T + T": (1, 1), "order 13: T + 12 T": (1, 12), "order 13: 6 T + 7 T": (6, 7)}[kind]
        p, q, want = jac(pool.tm[i], pool.z(), ks()), jac(pool.tm[j], pool.z(), ks()), pool.tm[(i + j) % 13]
    else:
        raise KeyError(kind)
    assert all(c < 3 * P for c in p[:4] + q[:4]) and all(c < 10 * P for c in p[4:] + q[4:])  # add's row of the table

    def chk(o, want=want, same=same):
        if same is not None:
            need(o == jwords(same), "an operand at infinity must give the other as it is")
        check_point(o, B_MADD if same is not None else B_ADD, want)
    return Case("g2_add", jwords(p) + jwords(q), chk, kind + (" at the top" if hi else ""), kind)


def add_blocks(pool, rnd):
    cases = [add_case(pool, kind, i & 1, rnd) for kind in ADD_KINDS for i in range(8 if kind != "generic" else 80)]
    return {"g2_add/mixed": mix(cases, rnd),
            "g2_add/uniform": uniform([(k, [add_case(pool, k, i & 1, rnd) for i in range(64)]) for k in ("P + P", "P - P", "infinity + Q")])}


def dbl_blocks(pool, rnd):
    def one(kind, hi, comps=None):
        a = pool.pt()
        p = comps(a) if comps else jac(a, pool.z(), pool.ks(TOP_DBL, hi))
        assert all(c < 15 * P for c in p[:4]) and all(c < 21 * P for c in p[4:])  # dbl's row of the table
        return Case("g2_dbl", jwords(p), lambda o, want=aff_add(a, a): check_point(o, B_DBL, want), kind, kind)

    def pattern(a):
        # Y and Z with limbs 0..12 all ones / all zero under the largest top limb their bounds admit
        low = rnd.choice((LOW_ONES, 0))
        v = ((rnd.choice((1, (21 * P >> 364) - 1))) << 364) | low
        zc = (v * RINV % P, rnd.randrange(P))
        p = jac(a, zc, [14, 14, 14, 14, 0, 20])
        p[4] = v
        return p

    cases = [one("generic", 0) for _ in range(60)] + [one("top", 1) for _ in range(40)] + [one("pattern", 1, pattern) for _ in range(24)]
    t_cases = []
    for i in range(16):
        t = pool.tm[1 + i % 12]
        p = jac(t, pool.z(), pool.ks(TOP_DBL, i & 1))
        t_cases.append(Case("g2_dbl", jwords(p), lambda o, want=aff_add(t, t): check_point(o, B_DBL, want), "order 13", "order 13"))
    return {"g2_dbl/mixed": mix(cases + t_cases, rnd), "g2_dbl/uniform": uniform([("top", [one("top", 1) for _ in range(64)])])}


def fedback_cases(pool, rnd):
    """P, Q, an affine R -> the outputs of dbl, madd and add into add (every ordered pair), dbl and madd"""
    out = []
    for i in range(64):
        hi = i & 1
        a, b, r = pool.pt(), pool.pt(), pool.pt()
        form = i % 4
        if form == 2:
            b = r = a  # P = Q = R: doublings everywhere
        elif form == 3:
            a, b, r = pool.tm[1 + i % 12], pool.tm[1 + (i // 4) % 12], pool.tm[1 + (i // 2) % 12]  # sums meet in the group of order 13
        p, q = jac(a, pool.z(), pool.ks(TOP_MADD, hi)), jac(b, pool.z(), pool.ks(TOP_MADD, hi))
        rr = [rep(c, 2 if hi else rnd.randrange(3)) for c in r[0] + r[1]]
        assert all(c < 3 * P for c in p[:4] + q[:4] + rr) and all(c < 10 * P for c in p[4:] + q[4:])
        o3 = [aff_add(a, a), aff_add(a, r), aff_add(a, b)]
        wants = [(aff_add(x, y), B_ADD) for x in o3 for y in o3]
        for x in o3:
            wants += [(aff_add(x, x) if x is not None else "skip", B_DBL), (aff_add(x, r), B_MADD)]

        def chk(o, wants=wants, o3=o3):
            for k, (want, bounds) in enumerate(wants):
                if want == "skip":  # dbl of infinity is outside dbl's contract
                    continue
                # a sum with an operand at infinity is the other operand as it is: madd's bounds at most
                i, j = divmod(k, 3) if k < 9 else (None, None)
                b = B_MADD if k < 9 and (o3[i] is None or o3[j] is None) else bounds
                check_point(o[84 * k:84 * k + 84], b, want, "output %d" % k)
        out.append(Case("g2_fedback", jwords(p) + jwords(q) + [w for c in rr for w in nl(c)], chk, "form %d" % form))
    return out


def conv_cases(pool, rnd):
    blocks = {}
    out = []
    for i in range(70):
        a = pool.pt() if i % 5 else pool.tm[1 + i % 12]
        p = [0] * 6 if i in (3, 40) else jac(a, pool.z() if i % 7 else (1, 0), pool.ks(TOP_AFF, i & 1))
        if i == 5:
            p = [rnd.randrange(15 * P) for _ in range(4)] + [0, 0]  # the identity with junk in X and Y
        want = None if p[4:] == [0, 0] else a
        assert all(c < 15 * P for c in p)

        def chk(o, want=want):
            need(o[56] == (1 if want is None else 0), "flags %x" % o[56])
            for k in range(4):
                check_fe(o[14 * k:14 * k + 14], 1, residue=0 if want is None else (want[0] + want[1])[k], what="coordinate %d (canonical)" % k)
            if want is None:
                need(all(x == 0 for x in o[:56]), "infinity: x = y = 0")
        out.append(Case("g2_toaff", jwords(p), chk))
    blocks["g2_toaff"] = out
    fb, tb = [], []
    for i in range(70):
        a = pool.pt()
        z = (0, rnd.randrange(1, P)) if i == 7 else (rnd.randrange(1, P), 0) if i == 8 else pool.z()
        z2 = f2mul(z, z)
        c = list(f2mul(a[0], z2) + f2mul(a[1], f2mul(z2, z)) + z)
        if i in (2, 33):
            c[4] = c[5] = 0  # Z == 0: the identity, whatever X and Y hold
        m = [v * (1 << 384) % P for v in c]

        def chk(o, c=c):
            if c[4] == c[5] == 0:
                need(all(x == 0 for x in o), "the identity is all-zero")
                return
            for k in range(6):
                check_fe(o[14 * k:14 * k + 14], 2, residue=c[k], what="component %d" % k)
        fb.append(Case("g2_fromblst", [w for v in m for w in w32(v, 12)], chk))
        ks = [62] * 6 if i & 1 else [rnd.randrange(63) for _ in range(6)]
        p = [0] * 6 if i in (2, 33) else [rep(v, k) for v, k in zip(c, ks)]
        assert all(v < 64 * P for v in p)
        wantw = [w for v in p for w in w32(v * RINV % P * (1 << 384) % P, 12)]
        tb.append(Case("g2_toblst", jwords(p), lambda o, w=wantw: need(o == w, "not the canonical blst_p2")))
    blocks["g2_fromblst"], blocks["g2_toblst"] = fb, tb
    return blocks


# ------------------------------------------------------------------------------------------------ g2io
HALF = (P - 1) // 2
LEX_VALUES = [(0, 0), (1, 0), (HALF, 0), (HALF + 1, 0), (P - 1, 0), (None, 1), (None, HALF), (None, HALF + 1), (None, P - 1)]


def io_cases(pool, rnd):
    blocks = {}
    out = []
    for v in [0, P - 1, P, P + 1, 2 * P - 1, 2 * P, 1, (1 << 364) - 1, 1 << 364] + pattern_values(2) + [rnd.randrange(2 * P + 1) for _ in range(52)]:
        assert v <= 2 * P
        out.append(Case("io_canon2", nl(v), lambda o, w=v % P: check_fe(o, 1, exact=w), "%x.." % (v >> 350)))
    blocks["io_canon2"] = out
    out = []
    for c0, c1 in LEX_VALUES:
        for k in (0, 1, 2, 7, 62, 63, 1000, 2519):
            y = (rnd.randrange(P) if c0 is None else c0, c1)
            a = (rep(y[0], k), rep(y[1], (k * 7 + 1) % 2520))
            assert all(c < 2520 * P and all(x < 1 << 30 for x in nl(c)) for c in a)
            out.append(Case("io_lex", f2words(a), lambda o, w=int(CM.lex_largest(y)): need(o == [w], "verdict %s, expected %d" % (o, w)),
                            "c0 %s, c1 %x.., + %d p" % ("random" if c0 is None else hex(c0)[:8], c1 >> 350, k)))
    blocks["io_lex"] = out
    # sqrt
    out = []
    nonres = next(v for v in range(2, 50) if pow(v, HALF, P) == P - 1)
    vals = [((0, 0), "zero")]
    for _ in range(10):
        x = (rnd.randrange(P), rnd.randrange(P))
        vals.append((f2mul(x, x), "square"))
    while sum(1 for _, t in vals if t == "non-square") < 10:
        a = (rnd.randrange(P), rnd.randrange(P))
        if not CM.f2_is_square(a):
            vals.append((a, "non-square"))
    for v in (1, 4, 9, rnd.randrange(1, P) ** 2 % P):
        vals.append(((v, 0), "purely real, a residue"))
    for v in (nonres, nonres * 4 % P, P - 1, nonres * pow(rnd.randrange(1, P), 2, P) % P):
        assert pow(v, HALF, P) == P - 1
        vals.append(((v, 0), "purely real, t == 0: a1 = 0 and s = -a0"))
    for v in (1, 2, P - 1, rnd.randrange(1, P)):
        vals.append(((0, v), "purely imaginary"))
    for a, tag in vals:
        for ks in ((0, 0), (63, 63), (rnd.randrange(64), rnd.randrange(64))):
            ar = (rep(a[0], ks[0]), rep(a[1], ks[1]))
            assert all(c < 64 * P for c in ar)

            def chk(o, a=a):
                sq = CM.f2_is_square(a)
                need(o[0] == int(sq), "verdict %d, expected %d" % (o[0], sq))
                if sq:
                    check_f2(o[1:], (2, 2), what="root")
                    r = res2((value(o[1:15]), value(o[15:29])))
                    need(f2mul(r, r) == a, "root^2 != a")
            out.append(Case("io_sqrt", f2words(ar), chk, "%s + (%d, %d) p" % (tag, ks[0], ks[1])))
    blocks["io_sqrt"] = out
    # the catalogue through uncompress, in_g2 and compress
    un, ing, co = [], [], []
    for name, b, cls in G2E.catalogue():
        try:
            a, valid = CM.decode(b), True
        except ValueError:
            a, valid = None, False
        assert valid == (cls != 1)

        def chk_un(o, a=a, valid=valid):
            need(o[0] == int(valid), "verdict %d, expected %d" % (o[0], valid))
            if valid:
                need(o[1] == (1 if a is None else 0), "flags %x" % o[1])
                for k in range(4):
                    check_fe(o[2 + 14 * k:16 + 14 * k], 1, residue=0 if a is None else (a[0] + a[1])[k], what="coordinate %d (canonical)" % k)
        un.append(Case("io_uncompress", list(b), chk_un, name))
        if valid:
            e = [0] * 4 if a is None else [rep(c, 0) for c in a[0] + a[1]]
            ing.append(Case("io_ing2", [w for c in e for w in nl(c)] + [1 if a is None else 0],
                            lambda o, w=int(cls == 0): need(o == [w], "verdict %s, expected %d" % (o, w)), name))
            hi = len(co) & 1
            p = [rnd.randrange(15 * P) for _ in range(4)] + [0, 0] if a is None else jac(a, pool.z(), pool.ks(TOP_AFF, hi))
            assert all(c < 15 * P for c in p)
            co.append(Case("io_compress", jwords(p), lambda o, w=list(CM.compress(a)): need(o == w, "bytes differ"), name))
    i = 0
    while len(ing) < 64 or len(co) < 64:  # more points on the twist through the same checks
        a = pool.pt(i) if i % 3 else CM.mul(3 + i, CM.G2)
        i += 1
        ing.append(Case("io_ing2", [w for c in a[0] + a[1] for w in nl(rep(c, 0))] + [0], lambda o, w=int(CM.in_g2_psi(a)): need(o == [w], "verdict"), "pool"))
        co.append(Case("io_compress", jwords(jac(a, pool.z(), TOP_AFF)), lambda o, w=list(CM.compress(a)): need(o == w, "bytes differ"), "pool"))
    blocks["io_uncompress"], blocks["io_ing2"], blocks["io_compress"] = un, ing, co
    out = []
    for i in range(64):
        a = pool.pt(i) if i % 4 else pool.tm[1 + i % 12] if i % 8 else CM.mul(2 + i, CM.G2)
        want = CM.psi(a)
        out.append(Case("io_psi", [w for c in a[0] + a[1] for w in nl(rep(c, 0))],
                        lambda o, want=want: (check_f2(o[:28], (2, 2), want[0], what="psi x"), check_f2(o[28:], (2, 2), want[1], what="psi y"))))
    blocks["io_psi"] = out
    cx, cy = CM.psi_constants()
    wantc = CM.limbs28(cx[0]) + CM.limbs28(cx[1]) + CM.limbs28(cy[0]) + CM.limbs28(cy[1])
    assert cx[0] == 0
    blocks["io_psiconst"] = [Case("io_psiconst", [i], lambda o: need(o == wantc, "not the constants the model derives")) for i in range(64)]
    return blocks


# ------------------------------------------------------------------------------------------------ g2lc
class FixedBase:
    """k * A on Python integers: 8-bit windows over tables of affine multiples, summed in Jacobian coordinates with ONE
    inversion per term"""

    def __init__(self, a):
        self.tab = []
        base = a
        for _ in range(32):
            row, acc = [None], None
            for _ in range(255):
                acc = aff_add(acc, base)
                row.append(acc)
            self.tab.append(row)
            base = aff_add(acc, base)

    def mul(self, k):
        acc = None  # (X, Y, Z) over Fp2
        for w in range(32):
            e = self.tab[w][(k >> (8 * w)) & 255]
            if e is not None:
                acc = jmadd(acc, e)
        return jaffine(acc)


def jaffine(j):
    if j is None:
        return None
    zi = f2inv(j[2])
    zi2 = f2mul(zi, zi)
    return f2mul(j[0], zi2), f2mul(j[1], f2mul(zi2, zi))


def jmadd(j, e):
    """Jacobian + affine on Fp2 pairs (the textbook mixed addition); the exceptional cases through the affine law"""
    if j is None:
        return (e[0], e[1], (1, 0))
    x1, y1, z1 = j
    zz = f2mul(z1, z1)
    h = f2sub(f2mul(e[0], zz), x1)
    r = f2sub(f2mul(e[1], f2mul(zz, z1)), y1)
    if h == (0, 0):
        s = aff_add(jaffine(j), e)
        return None if s is None else (s[0], s[1], (1, 0))
    hh = f2mul(h, h)
    hhh = f2mul(hh, h)
    v = f2mul(x1, hh)
    x3 = f2sub(f2sub(f2mul(r, r), hhh), f2add(v, v))
    return x3, f2sub(f2mul(r, f2sub(v, x3)), f2mul(y1, hhh)), f2mul(z1, h)


def thinned_scalars():
    """scalar_cases() with the 2^k - 1, 2^k, 2^k + 1 family kept at every eighth k"""
    fam = S.family_2k()
    return [k for k in S.scalar_cases() if k not in fam or fam[k] % 8 == 0]


def term_case(pt_aff, z, k, want, kind):
    if pt_aff is None:
        c = [5, 7, 11, 13, 0, 0]  # Z == 0: the identity, junk elsewhere
    else:
        z2 = f2mul(z, z)
        c = list(f2mul(pt_aff[0], z2) + f2mul(pt_aff[1], f2mul(z2, z)) + z)
    assert 0 <= k < R_FR and all(v < P for v in c)  # canonical blst_p2, a scalar below r
    words = [w for v in c for w in w32(v * (1 << 384) % P, 12)] + w32(k * (1 << 256) % R_FR, 8)
    return Case("lc_term", words, lambda o, want=want: check_point(o, B_MADD, want), "%d-bit scalar, %s" % (k.bit_length(), kind), kind)


def term_blocks(pool, rnd):
    base = pool.g[1]
    fb = FixedBase(base)
    cases = []
    scal = S.scalar_cases()
    for k in scal:  # every scalar case over a generator multiple with Z != 1
        kind = "zero scalar" if k == 0 else "short" if k.bit_length() <= 16 else "long" if k.bit_length() >= 250 else "generic"
        cases.append(term_case(base, pool.z(), k, fb.mul(k), kind))
    assert fb.mul(R_FR - 1) == neg_pt(base) and fb.mul(7) == CM.mul(7, base)
    thin = thinned_scalars()
    assert 100 < len(thin) < 400
    for k in thin:  # the order-13 point (k mod 13 decides) and an identity
        cases.append(term_case(pool.t, pool.z(), k, pool.tm[k % 13], "order 13"))
        cases.append(term_case(None, None, k, None, "identity"))
    nw = (len(cases) + 24 + 63) // 64
    cases += [term_case(pool.g[i % 3], pool.z(), 0, None, "zero scalar") for i in range(max(24, nw))]
    mixed = mix(cases, rnd)
    for w in range(0, len(mixed), 64):  # neighbours with scalars of very different bit lengths
        kinds = {c.kind for c in mixed[w:w + 64]}
        assert {"short", "long", "zero scalar", "identity", "order 13", "generic"} <= kinds
    uni = uniform([("zero scalar", [term_case(pool.g[i % 3], pool.z(), 0, None, "zero scalar") for i in range(64)]),
                   ("identity", [term_case(None, None, thin[i], None, "identity") for i in range(64)]),
                   ("order 13", [term_case(pool.t, pool.z(), 13 * (thin[i + 20] // 13), None, "order 13") for i in range(64)]),
                   ("long", [term_case(base, pool.z(), R_FR - 1 - i, fb.mul(R_FR - 1 - i), "long") for i in range(64)])])
    return {"lc_term/mixed": mixed, "lc_term/uniform": uni}


def tree_blocks(pool, rnd):
    """64 cases of 64 slots each: terms (X, Y < 3, Z < 10) and sums, identities, equal and opposite points side by side"""
    def slot_set(form):
        pts = []
        for t in range(64):
            if form == 0:
                a = pool.pt()
            elif form == 1:  # slot t and slot t + 32 hold the same point, then opposite ones, then identities
                a = pool.pt(t % 32) if t % 32 < 12 else neg_pt(pool.pt(t)) if t >= 32 and t % 32 < 20 else pool.pt(t) if t % 32 < 20 else None if t % 3 else pool.pt()
            elif form == 2:  # equal terms: every addition of every level a doubling
                a = pool.pt(7)
            elif form == 3:  # the group of order 13
                a = pool.tm[rnd.randrange(14) % 13]
            else:
                a = None if rnd.random() < 0.3 else pool.pt()
            pts.append(a)
        return pts

    one, six = [], []
    for i in range(64):
        pts = slot_set(i % 5)
        hi = i & 1
        comps = [jac(a, pool.z(), pool.ks(TOP_MADD, hi)) for a in pts]
        assert all(c < 3 * P for p in comps for c in p[:4]) and all(c < 10 * P for p in comps for c in p[4:])
        words = [w for p in comps for w in jwords(p)]
        lvl = [aff_add(pts[t], pts[t + 32]) for t in range(32)]
        keep = [comps[t] if pts[t + 32] is None else comps[t + 32] if pts[t] is None else None for t in range(32)]

        def chk1(o, lvl=lvl, keep=keep):
            for t in range(32):
                if keep[t] is not None:
                    need(o[84 * t:84 * t + 84] == jwords(keep[t]), "slot %d: an operand at infinity must give the other as it is" % t)
                check_point(o[84 * t:84 * t + 84], B_MADD if keep[t] is not None else B_ADD, lvl[t], "slot %d" % t)
        one.append(Case("lc_tree1", words, chk1, "form %d" % (i % 5)))
        lv = list(pts)
        half = 32
        while half:
            lv = [aff_add(lv[t], lv[t + half]) for t in range(half)]
            half >>= 1
        six.append(Case("lc_tree6", words, lambda o, want=lv[0]: check_point(o, B_MADD, want, "slot 0"), "form %d" % (i % 5)))
    return {"lc_tree1": one, "lc_tree6": six}


# ------------------------------------------------------------------------------------------------ the blocks
_cache = {}


def all_cases():
    """block -> cases, in the order they are sent.  Case 1 of every block is the one a -DG2_CHECK_PLANT_ERROR build
    spoils.  Built once per process and not changed afterwards."""
    if "blocks" in _cache:
        return _cache["blocks"]
    rnd = random.Random(SEED)
    pool = Pool(rnd)
    blocks = {}
    for part in (fp_product_cases(rnd), fp_sub_cases(rnd), fp_misc_cases(rnd), f2_cases(rnd), dbl_blocks(pool, rnd), madd_blocks(pool, rnd),
                 tab_blocks(pool, rnd), add_blocks(pool, rnd), {"g2_fedback": fedback_cases(pool, rnd)}, conv_cases(pool, rnd),
                 io_cases(pool, rnd), term_blocks(pool, rnd), tree_blocks(pool, rnd)):
        assert not set(part) & set(blocks)
        blocks.update(part)
    per_op = {}
    for block, cases in blocks.items():
        op = op_of(block)
        nin = OPS[op][0]
        per_op[op] = per_op.get(op, 0) + len(cases)
        for c in cases:
            assert c.op == op and len(c.words) == nin and all(0 <= w < 1 << 32 for w in c.words), (block, len(c.words), nin)
    assert set(per_op) == set(OPS), set(OPS) ^ set(per_op)
    assert all(n >= 64 for n in per_op.values()), {op: n for op, n in per_op.items() if n < 64}
    assert all(per_op[op] >= 128 for op in POINT_OPS + ("lc_term",)), per_op
    assert any(len(c) % 64 for b, c in blocks.items() if b.endswith("/mixed"))  # a partial last wave
    assert {b for layer in LAYERS.values() for b in layer} == set(blocks)
    _cache["blocks"] = blocks
    return blocks


def cases_per_op(blocks):
    per_op = {}
    for block, cases in blocks.items():
        per_op[op_of(block)] = per_op.get(op_of(block), 0) + len(cases)
    return per_op


def encode(blocks):
    """the text the harness reads"""
    parts = []
    for block, cases in blocks.items():
        parts.append("%s %d\n" % (op_of(block), len(cases)))
        parts += [" ".join("%x" % w for w in c.words) + "\n" for c in cases]
    return "".join(parts)


def decode(text, blocks):
    """what the harness printed -> block -> list of word lists; raises on anything but the expected shape: as many
    lines as cases, every line as long as the op's output"""
    lines = text.split("\n")
    pos = 0
    outs = {}
    for block, cases in blocks.items():
        op = op_of(block)
        assert lines[pos] == "%s %d" % (op, len(cases)), "block header %r, expected %s %d" % (lines[pos][:80], op, len(cases))
        pos += 1
        got = []
        for _ in cases:
            words = [int(x, 16) for x in lines[pos].split()]
            assert len(words) == OPS[op][1], "%s: %d words in a line, expected %d" % (op, len(words), OPS[op][1])
            got.append(words)
            pos += 1
        outs[block] = got
    assert lines[pos] == "done", "no end marker"
    return outs


def failures(blocks, outs):
    """[(block, case index, message)] for every case whose checker objects"""
    bad = []
    for block, cases in blocks.items():
        assert len(outs[block]) == len(cases)
        for i, (c, o) in enumerate(zip(cases, outs[block])):
            try:
                c.check(o)
            except AssertionError as e:
                bad.append((block, i, "%s%s" % (c.tag + ": " if c.tag else "", e)))
    return bad
