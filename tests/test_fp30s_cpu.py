"""fp30s.hip.h and g1_30s.hip.h — Fp in 13 signed 30-bit limbs and the addition chain of k_fbw_accum over it — compiled
for the host and held to Python integers.

  products     mul, sqr, mul2 on operands with every limb 0..11 at +(2^29 - 1) / -2^29 in the sign patterns that make a
               column largest (all products of one sign), on "unsigned" first operands (limbs 2^30 - 1), and on random
               ones: the result is congruent to the product / 2^390, centred, inside the documented interval;
  conversions  from28 / to28 and the round trip on 0, 1, p - 1 and random values; carry; is_zero_mod_p;
  chain_add    g1s::chain_add against g1::chain_add (fp28) on the same slots and against the chord / tangent formulas,
               as canonical affine points after g1s::to_xyzz28 (the u = 2 map out; from28 is the map in), with the input
               families of test_madd_forms_cpu.py: random sums spread over the state's intervals, extreme limbs of Y1
               and of the table's y, chains from empty, P + P, P - P, cancellation then re-use, tiny top limbs.
Every accumulator the new addition leaves is checked against the state's limb and value bounds (g1_30s.hip.h), and
every converted partial sum against the bounds k_blocksum expects (X < 10p, Y < 6p, ZZ, ZZZ < 2p, normalized)."""
import os
import random
import shutil
import subprocess

import pytest

import fp30s_model as M
from test_madd_forms_cpu import EMPTY, AFFINE, XYZZ, P, R384INV, affine_add, curve_point, limbs as limbs28, mont as mont28, neg, value as value28

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R390 = 1 << 390
R390INV = pow(R390, -1, P)
H = 1 << 29

HARNESS = r'''
#include <cstdio>
#include <cstring>
#include "g1_30s.hip.h"
using fp30s::Fe;
static Fe rd() { Fe r; for (int i = 0; i < 13; ++i) if (scanf("%d", &r.v[i]) != 1) r.v[i] = 0; return r; }
static fp28::Fe rd28() { fp28::Fe r; for (int i = 0; i < 14; ++i) if (scanf("%x", &r.v[i]) != 1) r.v[i] = 0; return r; }
static void raw(const Fe& a) { for (int i = 0; i < 13; ++i) printf("%d ", a.v[i]); }
static void raw28(const fp28::Fe& a) { for (int i = 0; i < 14; ++i) printf("%x ", a.v[i]); }
static void blst(const fp28::Fe& a) { ff::Fp c = fp28::to_blst(a); for (int i = 0; i < 12; ++i) printf("%x ", c.v[i]); }
int main() {
    const fp30s::Seeds sd = fp30s::seeds();
    char op[16];
    g1s::Xyzz acc;
    g1::Xyzz ref;
    g1s::set_inf(acc);
    g1::set_inf(ref);
    ff::u32 st = g1::CHAIN_EMPTY, st_ref = g1::CHAIN_EMPTY;
    while (scanf("%15s", op) == 1) {
        if (!strcmp(op, "mul")) { Fe a = rd(), b = rd(); raw(fp30s::mul(a, b, sd)); }
        else if (!strcmp(op, "sqr")) { Fe a = rd(); raw(fp30s::sqr(a, sd)); }
        else if (!strcmp(op, "mul2")) { Fe a = rd(), b = rd(), c = rd(), d = rd(); raw(fp30s::mul2(a, b, c, d, sd)); }
        else if (!strcmp(op, "carry")) { Fe a = rd(); raw(fp30s::carry(a)); }
        else if (!strcmp(op, "iszero")) { Fe a = rd(); printf("%d", (int)fp30s::is_zero_mod_p(a)); }
        else if (!strcmp(op, "from28")) { fp28::Fe a = rd28(); raw(fp30s::from28(a)); }
        else if (!strcmp(op, "to28")) { Fe a = rd(); raw28(fp30s::to28(a)); }
        else if (!strcmp(op, "const")) { raw(fp30s::one()); raw(fp30s::p_fe()); }
        else if (!strcmp(op, "set")) {  // state, x y zzz zz of the fp30s accumulator; the fp28 reference is not used after it
            if (scanf("%u", &st) != 1) return 1;
            acc.x = rd(); acc.y = rd(); acc.zzz = rd(); acc.zz = rd();
            st_ref = 99;
            printf("ok");
        } else if (!strcmp(op, "reset")) {
            g1s::set_inf(acc); g1::set_inf(ref); st = st_ref = g1::CHAIN_EMPTY;
            printf("ok");
        } else if (!strcmp(op, "add")) {
            unsigned m;
            if (scanf("%u", &m) != 1) return 1;
            const fp28::Fe x2 = rd28(), y2 = rd28();
            g1s::chain_add(acc, st, x2, y2, m ? 0xffffffffu : 0u, sd);
            if (st_ref != 99) g1::chain_add(ref, st_ref, x2, y2, m ? 0xffffffffu : 0u);
            g1::Xyzz out;
            g1s::to_xyzz28(out, acc, st, sd);
            printf("%u %u ", st, st_ref);
            raw(acc.x); raw(acc.y); raw(acc.zzz); raw(acc.zz);
            raw28(out.x); raw28(out.y); raw28(out.zzz); raw28(out.zz);
            blst(out.x); blst(out.y); blst(out.zzz); blst(out.zz);
            if (st_ref != 99) { blst(ref.x); blst(ref.y); blst(ref.zzz); blst(ref.zz); }
        } else return 1;
        printf("\n");
    }
    return 0;
}
'''


def build(tmp_path, exact=False, extra=()):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "fp30s_check.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / ("fp30s_check" + ("_exact" if exact else ""))
    subprocess.check_call([cxx, "-O1", "-std=c++17"] + (["-DKZGAMD_FORCE_EXACT_TESTS"] if exact else []) + list(extra) +
                          ["-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    return exe


def run(exe, lines):
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(lines)
    return out


def fmt(l):
    return " ".join(str(v) for v in l)


def fmt28(l):
    return " ".join("%x" % v for v in l)


def assert_centred(l, what=""):
    assert all(-H <= v < H for v in l[:12]), "not centred " + what


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("fp30s"))


def test_constants(exe):
    t = [int(v) for v in run(exe, ["const"])[0].split()]
    assert M.value(t[:13]) == R390 % P - (P if R390 % P > P // 2 else 0) and M.value(t[13:]) == P
    assert_centred(t[:13]) and assert_centred(t[13:])
    assert t[13:] == M.P_LIMBS
    assert P * 0x30003 % (1 << 32) == 1


def test_bounds_model_holds_and_gives_the_figures_the_headers_quote():
    """tests/fp30s_model.py, check_chain_add: the propagation of limb bounds and value intervals through mul, sqr, mul2
    and every step of g1s::chain_add, the doubling and the way back.  It asserts on its way that no column bound
    reaches 2^63, no carry pass sees a limb over 3 * 2^29 and no value leaves the interval its consumer documents; here
    the figures fp30s.hip.h, g1_30s.hip.h and NOTES section 34 quote are held to what it returns."""
    import math
    rep = M.check_chain_add()
    cols = {k: v for k, v in rep.items() if isinstance(v, int)}
    assert len(cols) >= 20 and all(v < M.LIMIT for v in cols.values())
    # two centred operands: 2^62.19; an operand with limbs up to 2^30 against a centred one, and mul2: 2^62.92
    wide = {"U2 = x2 * ZZ1", "S2 = y2 * ZZZ1", "Q = X1 * PP", "Y3 = R * V - Y1 * PPP", "dbl: Y3", "to_xyzz28: X",
            "mul, first operand with limbs up to 2^30", "mul2, centred operands below 64p"}
    for name, v in cols.items():
        assert "%.2f" % math.log2(v) == ("62.92" if name in wide else "62.19"), (name, math.log2(v))
    assert "%.2f" % math.log2(max(cols.values())) == "62.92"
    for state in ("affine", "xyzz"):
        assert rep["|X3|/p, " + state] < M.BOUND_X and rep["|Y3|/p, " + state] < M.BOUND_YZ
    assert "%.2f" % max(rep["|X3|/p, affine"], rep["|X3|/p, xyzz"]) == "2.03"
    assert "%.2f" % max(rep["|Y3|/p, affine"], rep["|Y3|/p, xyzz"]) == "0.52"
    # the operand rule of fp30s.hip.h in its own words: the sum of |p_j| * 2^29 is below 6.21 * 2^58
    assert sum(abs(v) for v in M.P_LIMBS) * M.H < 6.21 * 2 ** 58


def product_cases(rnd):
    """(kind, operands): the model's worst-case limb patterns, then random ones"""
    cases = [(k, ops) for k, ops, _ in M.worst_case_products()]
    for _ in range(400):
        k = rnd.choice(["mul", "mul_u", "sqr", "mul2"])
        n = {"mul": 2, "mul_u": 2, "sqr": 1, "mul2": 4}[k]
        ops = [M.centred(rnd.randrange(-2 * P, 2 * P)) for _ in range(n)]
        if k == "mul_u":
            ops[0] = M.unsigned(rnd.randrange(P))
        cases.append((k, ops))
    return cases


def test_products_against_python_integers(exe):
    rnd = random.Random(0x30)
    cases = product_cases(rnd)
    lines = [{"mul": "mul", "mul_u": "mul", "sqr": "sqr", "mul2": "mul2"}[k] + " " + " ".join(fmt(o) for o in ops) for k, ops in cases]
    assert len(cases) > 440
    for (k, ops), ln in zip(cases, run(exe, lines)):
        r = [int(v) for v in ln.split()]
        v = [M.value(o) for o in ops]
        prod = v[0] * v[0] if k == "sqr" else v[0] * v[1] + (v[2] * v[3] if k == "mul2" else 0)
        assert_centred(r, k)
        assert (M.value(r) * R390 - prod) % P == 0, k
        # the quotient is a centred 390-bit number: |m| <= 2^389 (1 + 2^-29)
        assert abs(M.value(r) * R390 - prod) <= ((1 << 389) + (1 << 361)) * P, k
        assert r == M.mont_product(k, ops)[0], k  # limb for limb what the model computes (and bounds)


def test_carry_and_zero_test(exe):
    rnd = random.Random(0x31)
    lazy = []
    for it in range(300):
        top = 3 * H if it % 3 == 0 else rnd.choice([H, 2 * H, 3 * H])
        l = [rnd.choice([-top, top, rnd.randrange(-top, top + 1)]) for _ in range(12)] + [rnd.randrange(-(1 << 25), 1 << 25)]
        if it < 4:
            l = [(-top if it & 1 else top)] * 12 + [(1 << 25) * (1 - (it & 2))]
        lazy.append(l)
    for l, ln in zip(lazy, run(exe, ["carry " + fmt(l) for l in lazy])):
        r = [int(v) for v in ln.split()]
        assert_centred(r)
        assert M.value(r) == M.value(l) and r == M.carry(l)
    zs = []
    for it in range(400):
        k = rnd.randrange(-31, 32)
        v = k * P + (0 if it % 2 == 0 else rnd.choice([1, -1, 1 << 30, -(1 << 30), 1 << 360, 3 << 30, rnd.randrange(1, P)]))
        l = M.centred(v) if it % 4 < 2 else M.lazy_split(v, rnd)
        zs.append((v % P == 0, l))
    for ex in (exe, build(exe.parent, exact=True)):
        for (want, l), ln in zip(zs, run(ex, ["iszero " + fmt(l) for _, l in zs])):
            assert int(ln) == int(want), (l, want)


def test_conversions_28_30(exe):
    rnd = random.Random(0x32)
    vals = [0, 1, P - 1, P, 2 * P - 1, (1 << 381) - 1, (1 << 364) - 1, (1 << 360), (1 << 360) - 1] + [rnd.randrange(2 * P) for _ in range(300)]
    out = run(exe, ["from28 " + fmt28(limbs28(v)) for v in vals])
    fe = []
    for v, ln in zip(vals, out):
        r = [int(x) for x in ln.split()]
        assert all(0 <= x < 1 << 30 for x in r[:12]) and r[12] >= 0 and M.value(r) == v
        assert r == M.unsigned(v)
        fe.append(r)
    # back: from the unsigned limbs, from centred limbs of the same value, and from lazy limbs (value >= 0)
    back = fe + [M.centred(v) for v in vals] + [M.lazy_split(v + P, rnd) for v in vals]
    want = vals + vals + [v + P for v in vals]
    for v, ln in zip(want, run(exe, ["to28 " + fmt(l) for l in back])):
        assert [int(x, 16) for x in ln.split()] == limbs28(v)


# ---- chain_add ----
def affine_of(words):
    v = [sum(w << (32 * i) for i, w in enumerate(words[12 * k:12 * k + 12])) for k in range(4)]
    assert all(c < P for c in v)
    x, y, zzz, zz = [c * R384INV % P for c in v]
    if zz == 0:
        assert x == 0 and y == 0 and zzz == 0
        return None
    return x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P


def rep30(val, k, rnd, form):
    """limbs of the 2^390-Montgomery residue of the field element val plus k * p (k may be negative)"""
    v = val * R390 % P
    v += (k - (v > P // 2)) * P  # the residue nearest zero, plus k * p
    return M.centred(v) if form == "centred" else M.lazy_pair(v, rnd)


class Script:
    def __init__(self, rnd):
        self.rnd, self.lines, self.checks, self.cur = rnd, [], [], None

    def reset(self):
        self.lines.append("reset")
        self.checks.append(None)
        self.cur = None

    def set_sum(self, aff, z=None, extreme_y=None):
        """a sum holding aff = (x, y) of E, i.e. (4x, 8y) on E', spread over the intervals of CHAIN_XYZZ"""
        rnd = self.rnd
        z = z or rnd.randrange(1, P)
        zz, zzz = z * z % P, z * z * z % P
        x = rep30(4 * aff[0] * zz % P, rnd.choice([-1, 0, 1]), rnd, "lazy")
        y = extreme_y or rep30(8 * aff[1] * zzz % P, 0, rnd, "centred")
        fe = [x, y, rep30(zzz, 0, rnd, "centred"), rep30(zz, 0, rnd, "centred")]
        for f in fe[1:]:
            assert abs(M.value(f)) < M.BOUND_YZ * P
        self.lines.append("set %d %s" % (XYZZ, " ".join(fmt(f) for f in fe)))
        self.checks.append(None)
        self.cur = aff

    def add(self, tag, m, pt, y_limbs=None, state=None, forms_only=False):
        self.lines.append("add %d %s %s" % (m, fmt28(limbs28(mont28(pt[0]))), fmt28(y_limbs or limbs28(mont28(pt[1])))))
        signed = neg(pt) if m else pt
        want = affine_add(self.cur, signed)
        self.checks.append((tag, "forms-only" if forms_only else want, state))
        self.cur = want


def build_script(rnd):
    s = Script(rnd)
    # random: onto sums spread over the state's intervals, onto single points, from empty; both signs
    for it in range(250):
        a, b = curve_point(rnd), curve_point(rnd)
        m = it & 1
        s.set_sum(a)
        s.add("random sum", m, b, state=XYZZ)
        s.add("random sum, then", m ^ 1, curve_point(rnd), state=XYZZ)
        s.reset()
        s.add("first point", m, a, state=AFFINE)
        s.add("second point", it >> 1 & 1, b, state=XYZZ)
        s.add("third point", m, curve_point(rnd), state=XYZZ)
    # extreme limbs of Y1 (all -2^29 or all 2^29 - 1, a top limb that keeps the value inside the interval) and of the
    # table's y (28-bit limbs all ones / all zero, which re-slice to 30-bit limbs all ones / all zero)
    for it in range(64):
        lo = [(-H if it & 1 else H - 1)] * 12
        y1 = lo + [rnd.randrange(-(1 << 19), 1 << 19) - (M.value(lo + [0]) >> 360)]
        assert abs(M.value(y1)) < M.BOUND_YZ * P
        z = rnd.randrange(1, P)
        aff = (rnd.randrange(P), M.value(y1) * R390INV * pow(8 * z * z * z, -1, P) % P)
        yl = ([(1 << 28) - 1] * 13 if it & 2 else [0] * 13) + [rnd.choice([0, 1, 0x1a010])]
        tab = (rnd.randrange(P), value28(yl) * pow(1 << 392, -1, P) % P)
        s.set_sum(aff, z=z, extreme_y=y1)
        s.add("extreme Y1, y2", it >> 2 & 1, tab, y_limbs=yl, state=XYZZ)
        s.reset()
        s.add("extreme y2 first", it >> 2 & 1, tab, y_limbs=yl, state=AFFINE)
        s.add("extreme y2 first, then", it >> 3 & 1, curve_point(rnd), state=XYZZ)
        s.reset()
        s.add("point", 0, curve_point(rnd), state=AFFINE)
        s.add("extreme y2 onto a point", it >> 2 & 1, tab, y_limbs=yl, state=XYZZ)
    # chains from empty: P + P, P - P, equal x with another y, cancellation then re-use, on a point and on a sum
    for it in range(40):
        a, b, c = curve_point(rnd), curve_point(rnd), curve_point(rnd)
        for m in (0, 1):
            s.reset()
            s.add("start: first", m, a, state=AFFINE)
            s.add("start: equal -> double", m, a, state=XYZZ)
            s.add("start: onto the double", m ^ 1, b, state=XYZZ)
            s.reset()
            s.add("start: first", m, a, state=AFFINE)
            s.add("start: opposite -> infinity", m ^ 1, a, state=EMPTY)
            s.add("start: after infinity", m, b, state=AFFINE)
            s.add("start: second after infinity", 0, c, state=XYZZ)
            s.reset()
            s.add("start: first", 0, a, state=AFFINE)
            s.add("start: equal x, other y", m, (a[0], (a[1] + 1 + it) % P), state=EMPTY, forms_only=True)
            s.cur = None
            s.add("start: after that", m, b, state=AFFINE)
        ab = affine_add(a, b)
        s.reset()
        s.add("sum: first", 0, a, state=AFFINE)
        s.add("sum: second", 0, b, state=XYZZ)
        s.add("sum: equal -> double", 0, ab, state=XYZZ)
        s.add("sum: equal to the negated point -> double", 1, neg(affine_add(ab, ab)), state=XYZZ)
        s.add("sum: opposite -> infinity", 1, affine_add(affine_add(ab, ab), affine_add(ab, ab)), state=EMPTY)
        s.add("sum: after infinity", 1, c, state=AFFINE)
        s.add("sum: second after infinity", 1, a, state=XYZZ)
        s.set_sum(a)
        s.add("sum over the intervals: equal -> double", 0, a, state=XYZZ)
        s.set_sum(a)
        s.add("sum over the intervals: opposite -> infinity", 1, a, state=EMPTY)
    # tiny top limbs of the table's y
    for it in range(80):
        yl = [rnd.randrange(1 << 28) for _ in range(13)] + [it & 1]
        if it % 10 == 0:
            yl = [0] * 13 + [it & 1]
        tiny = (rnd.randrange(P), value28(yl) * pow(1 << 392, -1, P) % P)
        m = it >> 1 & 1
        s.reset()
        s.add("tiny y2 first", m, tiny, y_limbs=yl, state=AFFINE)
        s.add("tiny y2 first, then", m, curve_point(rnd), state=XYZZ)
        s.add("tiny y2 onto a sum", m, tiny, y_limbs=yl, state=None)
    return s


def check_state(st, fe):
    x, y, zzz, zz = fe
    if st == EMPTY:
        assert all(v == 0 for f in fe for v in f)
        return
    for f in (y, zzz, zz):
        assert_centred(f)
    if st == AFFINE:
        assert all(0 <= v < 1 << 30 for v in x[:12]) and 0 <= M.value(x) < P and abs(M.value(y)) < 2 * P
        assert zz == M.ONE and zzz == M.ONE
    else:
        assert all(abs(v) < 1 << 30 for v in x[:12]) and abs(M.value(x)) < M.BOUND_X * P
        assert all(abs(M.value(f)) < M.BOUND_YZ * P for f in (y, zzz, zz)) and M.value(zz) % P


@pytest.mark.parametrize("exact", [False, True])
def test_chain_add_against_fp28_and_the_affine_formulas(tmp_path, exact):
    s = build_script(random.Random(0x30ADD))
    out = run(build(tmp_path, exact=exact), s.lines)
    seen = set()
    n = 0
    for chk, ln in zip(s.checks, out):
        if chk is None:
            continue
        tag, want, state = chk
        t = ln.split()
        st, st_ref = int(t[0]), int(t[1])
        fe = [[int(v) for v in t[2 + 13 * k:15 + 13 * k]] for k in range(4)]
        out28 = [[int(v, 16) for v in t[54 + 14 * k:68 + 14 * k]] for k in range(4)]
        words = [int(v, 16) for v in t[110:]]
        try:
            check_state(st, fe)
            bx, by, bzzz, bzz = [value28(f) for f in out28]
            assert all(v <= (1 << 28) - 1 for f in out28 for v in f[:13]), "partial sum not normalized"
            assert bx < 10 * P and by < 6 * P and bzz < 2 * P and bzzz < 2 * P
            got = affine_of(words[:48])
            if st_ref != 99:
                assert len(words) == 96 and st == st_ref, "state differs from g1::chain_add"
                assert got == affine_of(words[48:]), "differs from g1::chain_add (fp28)"
            if want != "forms-only":
                assert got == want, "differs from the affine formulas"
            if state is not None:
                assert st == state
            assert (got is None) == (st == EMPTY)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (tag, e))
        seen.add((tag.split(":")[0], st))
        n += 1
    assert n > 2500
    assert ("start", EMPTY) in seen and ("sum", EMPTY) in seen and ("extreme Y1, y2", XYZZ) in seen
