"""g1::chain_add (g1_28.hip.h), the addition k_fbw_accum inlines, compiled for the host and held to g1::madd, g1::dadd and
g1::dbl_affine — as canonical affine results (fp28::to_blst of every coordinate, divided in Python) — and to the
chord / tangent formulas in Python integers.

chain_add differs from madd in three ways, and each has its own edge: the sign of the table point goes into
R = 16p - Y1 +- S2 (8p - y1 +- y2 after a single table point) through a pad with two borrowed units per limb
(fp28::sub_signed_lazy), X3 = R^2 + 8p - 2Q - PPP takes
one carry pass over a pad with three (fp28::sub_2b_c), and a register beside the accumulator says whether it is empty,
one table point (the next addition is affine + affine, mmadd-2008-s) or a sum.  Inputs:
  random   accumulators spread over the documented bounds (X < 10p, Y < 6p, ZZ, ZZZ < 2p), curve points, both signs;
  pad      limbs 0..12 of Y1 and of S2 all 2^28 - 1 and all 0, in every combination, both signs, on a sum (S2 is a
           Montgomery product: y2 is solved for so that y2 * ZZZ1 * 2^-392 comes out as those limbs) and on a single
           table point (S2 = y2);
  start    chains from the empty accumulator: P + P, P - P, -P - P, equal x with another y, a sum that cancels to
           infinity and is added to again, on one table point and on a sum;
  tiny     y of the table point and Y of the accumulator with a top limb of 0 or 1.
Every output is checked against the bounds chain_add documents for the state it reports."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
M28 = (1 << 28) - 1
R392 = 1 << 392
RINV = pow(R392, -1, P)
R384INV = pow(1 << 384, -1, P)
EMPTY, AFFINE, XYZZ = 0, 1, 2
ONE = R392 % P
LOW_ONES = (1 << 364) - 1  # limbs 0..12 all 2^28 - 1


def limbs(v):
    """normalized representation: limbs 0..12 < 2^28, the rest in the top limb"""
    assert 0 <= v < 1 << 396
    return [(v >> (28 * i)) & M28 for i in range(13)] + [v >> 364]


def value(l):
    return sum(x << (28 * i) for i, x in enumerate(l))


def mont(v, k=0):
    """the Montgomery residue of the field element v, plus k * p"""
    return v * R392 % P + k * P


def curve_point(rnd):
    while True:
        x = rnd.randrange(P)
        rhs = (pow(x, 3, P) + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs and y:
            return x, (y if rnd.random() < 0.5 else P - y)


def affine_add(a, b):
    """chord / tangent (a = 0) formulas on field elements; None is infinity.  Identities of the field: the operands
    need not be on the curve."""
    if a is None:
        return b
    if b is None:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if (y1 + y2) % P == 0 or y1 != y2:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def neg(a):
    return None if a is None else (a[0], (P - a[1]) % P)


class Script:
    """lines for the harness and, per `add`, what to check on its output"""

    def __init__(self, rnd):
        self.rnd = rnd
        self.lines = []
        self.checks = []  # (tag, expected affine or "forms-only", expected state or None, is_doubling)
        self.cur = None   # the affine value of the accumulator the harness holds

    def set(self, st, aff, z=None, kx=0, ky=0, kzz=0, kzzz=0, y_limbs=None):
        """accumulator in state st holding the affine point aff; a sum is spread with z and the multiples of p"""
        if st == EMPTY:
            fe = [[0] * 14] * 4
        elif st == AFFINE:
            fe = [limbs(mont(aff[0])), y_limbs or limbs(mont(aff[1], ky)), limbs(ONE), limbs(ONE)]
        else:
            zz, zzz = z * z % P, z * z * z % P
            fe = [limbs(mont(aff[0] * zz, kx)), y_limbs or limbs(mont(aff[1] * zzz, ky)), limbs(mont(zzz, kzzz)), limbs(mont(zz, kzz))]
        self.lines.append("set %d %s" % (st, " ".join("%x" % v for f in fe for v in f)))  # x, y, zzz, zz
        self.cur = aff

    def add(self, tag, m, pt, y_limbs=None, state=None, forms_only=False):
        """acc +- pt; y_limbs overrides the Montgomery limbs of the table point's y (pt then names the same value)"""
        fe = limbs(mont(pt[0])) + (y_limbs or limbs(mont(pt[1])))
        self.lines.append("add %d %s" % (m, " ".join("%x" % v for v in fe)))
        signed = neg(pt) if m else pt
        dbl = self.cur is not None and self.cur == signed
        want = affine_add(self.cur, signed)
        self.checks.append((tag, "forms-only" if forms_only else want, state, dbl))
        self.cur = want


def field_of_y_limbs(l):
    return value(l) * RINV % P


def build_script(rnd):
    s = Script(rnd)
    # ---- random: sums over the documented bounds, single table points, both signs ----
    for it in range(300):
        a, b = curve_point(rnd), curve_point(rnd)
        m = it & 1
        s.set(XYZZ, a, z=rnd.randrange(1, P), kx=rnd.randrange(10), ky=rnd.randrange(6), kzz=rnd.randrange(2), kzzz=rnd.randrange(2))
        s.add("random sum", m, b, state=XYZZ)
        s.set(XYZZ, a, z=rnd.randrange(1, P), kx=9, ky=5, kzz=1, kzzz=1)  # the largest multiples the bounds admit
        s.add("random sum, largest", m, b, state=XYZZ)
        s.set(AFFINE, a, ky=rnd.randrange(2))
        s.add("random table point", m, b, state=XYZZ)
        s.set(EMPTY, None)
        s.add("first point", m, b, state=AFFINE)
    # ---- pad: limbs 0..12 of Y1 and S2 all ones / all zero ----
    for y1_low, y1_tops in ((LOW_ONES, (0, 1, 0x1a010, 0x34021, 0x9c065)), (0, (0, 1, 0x1a011, 0x34022, 0x9c066))):
        for s2_low, s2_tops in ((LOW_ONES, (0, 1, 0x1a010)), (0, (0, 1, 0x1a011))):
            for y1_top in y1_tops:
                for s2_top in s2_tops:
                    for m in (0, 1):
                        y1 = (y1_top << 364) | y1_low
                        s2 = (s2_top << 364) | s2_low
                        assert y1 < 6 * P and s2 < 2 * P
                        x1, x2 = rnd.randrange(P), rnd.randrange(P)
                        # a sum: Y1 as given, y2 solved so that the Montgomery product y2 * ZZZ1 * 2^-392 is s2 exactly.
                        # The product of a and b comes out in [ab / 2^392, ab / 2^392 + p): as s2 when s2 is in that
                        # range, else as s2 + p — for a tiny s2, ZZZ1 is drawn again until it is (a few per cent of
                        # the draws are)
                        if s2 < P:
                            for _ in range(5000):
                                z = rnd.randrange(1, P)
                                zzz_rep = mont(z * z * z % P, rnd.randrange(2))
                                y2_rep = s2 * R392 * pow(zzz_rep, -1, P) % P
                                if y2_rep * zzz_rep <= s2 * R392:
                                    break
                            assert (y2_rep * zzz_rep + (-y2_rep * zzz_rep * pow(P, -1, R392) % R392) * P) // R392 == s2
                            aff1 = (x1, y1 * RINV * pow(z * z * z, -1, P) % P)
                            s.set(XYZZ, aff1, z=z, kx=rnd.randrange(10), kzz=rnd.randrange(2), y_limbs=limbs(y1))
                            s.lines[-1] = _replace_zzz(s.lines[-1], limbs(zzz_rep))
                            s.add("pad sum y1=%x s2=%x" % (y1_top, s2_top), m, (x2, y2_rep * RINV % P), y_limbs=limbs(y2_rep), state=XYZZ)
                        # one table point: S2 = y2, Y1 = y or 2p - y of a table point (at most 2p)
                        if s2 < P and y1 <= 2 * P:
                            s.set(AFFINE, (x1, y1 * RINV % P), y_limbs=limbs(y1))
                            s.add("pad point y1=%x s2=%x" % (y1_top, s2_top), m, (x2, s2 * RINV % P), y_limbs=limbs(s2), state=XYZZ)
    # ---- start: the exceptional cases at the start of a chain and later ----
    for it in range(40):
        a, b, c = curve_point(rnd), curve_point(rnd), curve_point(rnd)
        for m in (0, 1):
            s.set(EMPTY, None)
            s.add("start: first", m, a, state=AFFINE)
            s.add("start: equal -> double", m, a, state=XYZZ)
            s.add("start: onto the double", m ^ 1, b, state=XYZZ)
            s.set(EMPTY, None)
            s.add("start: first", m, a, state=AFFINE)
            s.add("start: opposite -> infinity", m ^ 1, a, state=EMPTY)
            s.add("start: after infinity", m, b, state=AFFINE)
            s.add("start: second after infinity", 0, c, state=XYZZ)
            # equal x, another y (not a curve point: the formulas give infinity, as madd does)
            s.set(AFFINE, a)
            s.add("start: equal x, other y", m, (a[0], (a[1] + 1 + it) % P), state=EMPTY, forms_only=True)
            s.cur = None
            s.add("start: after that", m, b, state=AFFINE)
        # a sum that equals the next table point, and one that is its opposite
        ab = affine_add(a, b)
        s.set(EMPTY, None)
        s.add("sum: first", 0, a, state=AFFINE)
        s.add("sum: second", 0, b, state=XYZZ)
        s.add("sum: equal -> double", 0, ab, state=XYZZ)
        s.add("sum: equal to the negated point -> double", 1, neg(affine_add(ab, ab)), state=XYZZ)
        s.add("sum: opposite -> infinity", 1, affine_add(affine_add(ab, ab), affine_add(ab, ab)), state=EMPTY)
        s.add("sum: after infinity", 1, c, state=AFFINE)
        s.add("sum: second after infinity", 1, a, state=XYZZ)
        s.set(XYZZ, a, z=rnd.randrange(1, P), kx=rnd.randrange(10), ky=rnd.randrange(6), kzz=1, kzzz=1)
        s.add("sum over the bounds: equal -> double", 0, a, state=XYZZ)
        s.set(XYZZ, a, z=rnd.randrange(1, P), kx=rnd.randrange(10), ky=rnd.randrange(6), kzz=1, kzzz=1)
        s.add("sum over the bounds: opposite -> infinity", 1, a, state=EMPTY)
    # ---- tiny: top limbs of 0 and 1 in y2 and in Y1 ----
    for it in range(120):
        top = it & 1
        m = (it >> 1) & 1
        yl = [rnd.randrange(1 << 28) for _ in range(13)] + [top]
        if it % 12 == 0:
            yl = [0] * 13 + [top]
        tiny = (rnd.randrange(P), field_of_y_limbs(yl))
        a = curve_point(rnd)
        s.set(EMPTY, None)
        s.add("tiny y2 first", m, tiny, y_limbs=yl, state=AFFINE)  # 2p - y2 for m = 1
        s.add("tiny y2 first, then", m, a, state=XYZZ)
        s.set(AFFINE, a)
        s.add("tiny y2 onto a point", m, tiny, y_limbs=yl, state=XYZZ)
        s.set(XYZZ, a, z=rnd.randrange(1, P), kx=rnd.randrange(10), ky=rnd.randrange(6), kzz=rnd.randrange(2), kzzz=rnd.randrange(2))
        s.add("tiny y2 onto a sum", m, tiny, y_limbs=yl, state=XYZZ)
        z = rnd.randrange(1, P)
        s.set(XYZZ, (a[0], field_of_y_limbs(yl) * pow(z * z * z, -1, P) % P), z=z, kx=rnd.randrange(10), y_limbs=yl)
        s.add("tiny Y1 in a sum", m, curve_point(rnd), state=XYZZ)
        s.set(AFFINE, tiny, y_limbs=yl)
        s.add("tiny Y1 in a point", m, a, state=XYZZ)
    return s


def _replace_zzz(line, zzz_limbs):
    parts = line.split()
    parts[2 + 28:2 + 42] = ["%x" % v for v in zzz_limbs]
    return " ".join(parts)


HARNESS = r'''
#include <cstdio>
#include <cstring>
#include "g1_28.hip.h"
using fp28::Fe;
using g1::Xyzz;
static Fe rd() { Fe r; for (int i = 0; i < 14; ++i) if (scanf("%x", &r.v[i]) != 1) r.v[i] = 0; return r; }
static void raw(const Fe& a) { for (int i = 0; i < 14; ++i) printf("%x ", a.v[i]); }
static void blst(const Fe& a) { ff::Fp c = fp28::to_blst(a); for (int i = 0; i < 12; ++i) printf("%x ", c.v[i]); }
static void pt(const Xyzz& a) { blst(a.x); blst(a.y); blst(a.zzz); blst(a.zz); }
int main() {
    char op[8];
    Xyzz acc;
    g1::set_inf(acc);
    ff::u32 st = g1::CHAIN_EMPTY;
    while (scanf("%7s", op) == 1) {
        if (!strcmp(op, "set")) {
            if (scanf("%u", &st) != 1) return 1;
            acc.x = rd(); acc.y = rd(); acc.zzz = rd(); acc.zz = rd();
        } else if (!strcmp(op, "add")) {
            unsigned m;
            if (scanf("%u", &m) != 1) return 1;
            const Fe x2 = rd(), y2 = rd();
            const Fe ys = m ? fp28::neg<2>(y2) : y2;
            Xyzz a = acc, b = acc, q, d;
            g1::madd(a, x2, ys);
            g1::set_affine(q, x2, ys);
            g1::dadd(b, q);
            g1::dbl_affine(d, x2, ys);
            g1::chain_add(acc, st, x2, y2, m ? 0xffffffffu : 0u);
            printf("%u ", st);
            raw(acc.x); raw(acc.y); raw(acc.zzz); raw(acc.zz);
            pt(acc); pt(a); pt(b); pt(d);
            printf("\n");
        } else return 1;
    }
    return 0;
}
'''


def affine_of(words):
    """48 canonical blst words (x, y, zzz, zz) -> affine field elements, None for infinity"""
    v = [sum(w << (32 * i) for i, w in enumerate(words[12 * k:12 * k + 12])) for k in range(4)]
    assert all(c < P for c in v), "to_blst result not canonical"
    x, y, zzz, zz = [c * R384INV % P for c in v]
    if zz == 0:
        assert x == 0 and y == 0 and zzz == 0, "infinity is all-zero"
        return None
    return x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P


def check_bounds(st, fe):
    x, y, zzz, zz = fe
    for f in fe:
        assert all(l <= M28 for l in f[:13]), "not normalized"
    if st == EMPTY:
        assert all(l == 0 for f in fe for l in f), "infinity is all-zero limbs"
    elif st == AFFINE:
        assert value(x) < P and value(y) <= 2 * P and zzz == limbs(ONE) and zz == limbs(ONE)
    else:
        assert st == XYZZ
        assert value(x) < 10 * P and value(y) < 6 * P and value(zzz) < 2 * P and value(zz) < 2 * P
        assert value(zz) % P != 0


@pytest.mark.parametrize("exact", [False, True])
def test_chain_add_against_madd_dadd_dbl_affine_and_the_affine_formulas(tmp_path, exact):
    rnd = random.Random(0xADD5)
    s = build_script(rnd)
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "chaincheck.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "chaincheck"
    subprocess.check_call([cxx, "-O1", "-std=c++17"] + (["-DKZGAMD_FORCE_EXACT_TESTS"] if exact else []) +
                          ["-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], input="\n".join(s.lines) + "\n", capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(s.checks) > 2500
    seen = set()
    for (tag, want, state, dbl), ln in zip(s.checks, out):
        t = [int(x, 16) for x in ln.split()]
        st, fe, words = t[0], [t[1 + 14 * k:15 + 14 * k] for k in range(4)], t[57:]
        assert len(words) == 4 * 48, tag
        try:
            check_bounds(st, fe)
            got, by_madd, by_dadd = [affine_of(words[48 * k:48 * k + 48]) for k in range(3)]
            assert got == by_madd, "differs from g1::madd"
            assert got == by_dadd, "differs from g1::dadd"
            if dbl:
                assert got == affine_of(words[144:192]), "differs from g1::dbl_affine"
            if want != "forms-only":
                assert got == want, "differs from the affine formulas"
            if state is not None:
                assert st == state, "state %d, expected %d" % (st, state)
            assert (got is None) == (st == EMPTY)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (tag, e))
        seen.add((tag.split(":")[0].split(" y1=")[0], st, dbl))
    # the script reached what it set out to: doublings on a point and on a sum, infinities, all three states
    assert ("start", XYZZ, True) in seen and ("sum", XYZZ, True) in seen and ("start", EMPTY, False) in seen
    assert ("sum", EMPTY, False) in seen and ("pad sum", XYZZ, False) in seen and ("pad point", XYZZ, False) in seen


def test_pad_constants_are_multiples_of_p_with_the_borrowed_units(tmp_path):
    """fp28::padw<K, B>: value K * p, limbs 0..12 at least B * (2^28 - 1), top limb (K*p >> 364) - B — for the two pads
    chain_add uses, and padw<K, 1> against the pad_l<K> tables"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "padcheck.cpp"
    src.write_text(r'''
#include <cstdio>
#include "fp28.hip.h"
template <int K, int B> static void show() {
    constexpr fp28::PadW w = fp28::padw<K, B>();
    printf("%d %d", K, B);
    for (int i = 0; i < 14; ++i) printf(" %x", w.v[i]);
    printf("\n");
}
template <int K> static void table() {
    printf("%d 1", K);
    for (int i = 0; i < 14; ++i) printf(" %x", fp28::pad_l<K>(i));
    printf("\n");
}
int main() {
    show<16, 2>(); show<8, 2>(); show<8, 3>();
    show<2, 1>(); show<4, 1>(); show<8, 1>(); show<16, 1>(); show<32, 1>();
    table<2>(); table<4>(); table<8>(); table<16>(); table<32>();
    return 0;
}
''')
    exe = tmp_path / "padcheck"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"), str(src), "-o", str(exe)])
    rows = [[int(x, 16) if i >= 2 else int(x) for i, x in enumerate(ln.split())] for ln in subprocess.check_output([str(exe)], text=True).strip().split("\n")]
    assert len(rows) == 13
    for k, b, *l in rows:
        assert value(l) == k * P, (k, b)
        assert all(x >= b * M28 for x in l[:13]) and all(x < (b + 1) << 28 for x in l[:13]), (k, b)
        assert l[13] == (k * P >> 364) - b, (k, b)
    assert rows[3:8] == rows[8:13]
