"""g2_28.hip.h (Fp2 over fp28::Fe and G2 points, one value per lane) compiled for the host and held to host_pairing.h,
the specification: every Fp2 routine against f2_*, g2::dbl against g2_dbl, g2::madd / madd_complete against g2_add with
Z2 = 1, to_affine against g2_to_affine, the blst_p2 conversions against themselves — compared as canonical residues
inside one stand-alone program (its own main), and the bounds of every output checked here against the header's table.

Inputs:
  random   residues spread over the bound each routine documents (a Montgomery residue plus a random multiple of p);
  bound    the largest multiple the bound admits on every component;
  limbs    components whose limbs 0..12 are all 2^28 - 1, and all 0, under a top limb that keeps them inside the bound;
  points   curve points of E'(Fp2) with a random Z; for the additions P + P (reported as MADD_DOUBLE, and doubled by
           madd_complete), P - P (MADD_INF), an accumulator at infinity (the table point comes back), an equal x with
           another y (MADD_INF, as g2_add), all on accumulators at the top of their bounds too;
  table    g2::madd_tab, the step both walks of groupmul.hip are made of, against g2_add: an entry flagged as infinity
           (the accumulator must come back untouched, also when it is infinity itself), an entry added and subtracted,
           P + P, P - P, -P - P and an accumulator at infinity through the table form.
An affine operand at infinity is not an input of madd itself: madd_tab is where the flag is read.  On the GPU the same
cases arise from a G2 base of order 13, whose table has infinite entries (tests/test_group_mul_gpu.py).

A second build of the same program under UndefinedBehaviorSanitizer runs the same script once (nothing preloaded), and
groupmul.hip must cross-compile for gfx950 with the product's flags."""
import importlib.util
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-kzg_amd", "csrc")
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
M28 = (1 << 28) - 1
R392 = 1 << 392
LOW_ONES = (1 << 364) - 1
DONE, DOUBLE, INF = 0, 1, 2

PROGRAM = r'''
#include <cstdio>
#include <cstring>
#include "g2_28.hip.h"
#include "host_pairing.h"
namespace hp = kzgamd::pairing;
using fp28::Fe;
using g2::F2;
static bool rd(Fe& r) { for (int i = 0; i < 14; ++i) if (scanf("%x", &r.v[i]) != 1) return false; return true; }
static bool rd2(F2& r) { return rd(r.c0) && rd(r.c1); }
static void raw(const Fe& a) { for (int i = 0; i < 14; ++i) printf("%x ", a.v[i]); }
static void raw2(const F2& a) { raw(a.c0); raw(a.c1); }
static hp::Fp2 spec(const F2& a) { ff::Fp o[2]; g2::to_blst(o, a); return {o[0], o[1]}; }
static hp::G2Jac specj(const g2::Jac& p) { hp::G2Jac r; g2::to_blst_jacobian(reinterpret_cast<ff::Fp*>(&r), p); return r; }
static bool same(const hp::G2Jac& a, const hp::G2Jac& b) { return hp::f2_eq(a.x, b.x) && hp::f2_eq(a.y, b.y) && hp::f2_eq(a.z, b.z); }
int main() {
    char op[16];
    while (scanf("%15s", op) == 1) {
        if (op[0] == 'F') {  // F<name> a b
            F2 a, b, r = g2::zero();
            if (!rd2(a) || !rd2(b)) return 2;
            const hp::Fp2 sa = spec(a), sb = spec(b);
            hp::Fp2 want = hp::f2_zero();
            const char* n = op + 1;
            if (!strcmp(n, "add")) { r = g2::add(a, b); want = hp::f2_add(sa, sb); }
            else if (!strcmp(n, "dbl")) { r = g2::dbl(a); want = hp::f2_dbl(sa); }
            else if (!strcmp(n, "sub4")) { r = g2::sub<4>(a, b); want = hp::f2_sub(sa, sb); }
            else if (!strcmp(n, "sub8")) { r = g2::sub<8>(a, b); want = hp::f2_sub(sa, sb); }
            else if (!strcmp(n, "sub16")) { r = g2::sub<16>(a, b); want = hp::f2_sub(sa, sb); }
            else if (!strcmp(n, "sub32")) { r = g2::sub<32>(a, b); want = hp::f2_sub(sa, sb); }
            else if (!strcmp(n, "neg2")) { r = g2::neg<2>(a); want = hp::f2_neg(sa); }
            else if (!strcmp(n, "neg16")) { r = g2::neg<16>(a); want = hp::f2_neg(sa); }
            else if (!strcmp(n, "mul")) { r = g2::mul(a, b); want = hp::f2_mul(sa, sb); }
            else if (!strcmp(n, "sqr")) { r = g2::sqr(a); want = hp::f2_sqr(sa); }
            else if (!strcmp(n, "mulfe")) { r = g2::mul_fe(a, b.c0); want = hp::f2_mul_fp(sa, sb.c0); }
            else if (!strcmp(n, "red")) { r = g2::red(a); want = sa; }
            else if (!strcmp(n, "inv")) { r = g2::inv(a); want = hp::f2_inv(sa); }
            else if (!strcmp(n, "iszero")) { r.c0.v[0] = g2::is_zero(a); want = hp::f2_zero(); want.c0.v[0] = hp::f2_is_zero(sa); raw2(r); printf("%d\n", (int)(r.c0.v[0] == want.c0.v[0])); continue; }
            else return 3;
            raw2(r);
            printf("%d\n", (int)hp::f2_eq(spec(r), want));
        } else if (op[0] == 'D') {  // D X Y Z
            g2::Jac p;
            if (!rd2(p.x) || !rd2(p.y) || !rd2(p.z)) return 2;
            const hp::G2Jac want = hp::g2_dbl(specj(p));
            g2::dbl(p);
            raw2(p.x); raw2(p.y); raw2(p.z);
            printf("%d\n", (int)same(specj(p), want));
        } else if (op[0] == 'M') {  // M X Y Z x2 y2
            g2::Jac p;
            F2 x2, y2;
            if (!rd2(p.x) || !rd2(p.y) || !rd2(p.z) || !rd2(x2) || !rd2(y2)) return 2;
            const hp::G2Jac q = {spec(x2), spec(y2), hp::f2_one()};
            const hp::G2Jac want = hp::g2_add(specj(p), q);
            const g2::Jac orig = p;
            g2::Jac c = p;
            const unsigned st = g2::madd(p, x2, y2);
            g2::madd_complete(c, x2, y2);
            printf("%u ", st);
            raw2(c.x); raw2(c.y); raw2(c.z);
            bool ok = same(specj(c), want);
            if (st != g2::MADD_DOUBLE) ok = ok && same(specj(p), want);  // madd alone is the answer unless it says "double"
            else ok = ok && !memcmp(&p, &orig, sizeof p);                // ... and then it leaves p alone
            printf("%d\n", (int)ok);
        } else if (op[0] == 'T') {  // T X Y Z x2 y2 flags neg: one step of a table walk
            g2::Jac p;
            g2::AffPt e;
            unsigned neg;
            if (!rd2(p.x) || !rd2(p.y) || !rd2(p.z) || !rd2(e.x) || !rd2(e.y) || scanf("%x %x", &e.flags, &neg) != 2) return 2;
            e.pad[0] = e.pad[1] = e.pad[2] = 0;
            hp::G2Jac q = {spec(e.x), spec(e.y), hp::f2_one()};
            if (neg) q = hp::g2_neg(q);
            if (e.flags & 1) q = hp::g2_inf();
            const hp::G2Jac want = hp::g2_add(specj(p), q);
            const g2::Jac orig = p;
            g2::madd_tab(p, e, neg ? 0xffffffffu : 0u);
            printf("%u ", e.flags);
            raw2(p.x); raw2(p.y); raw2(p.z);
            bool ok = same(specj(p), want);
            if (e.flags & 1) ok = ok && !memcmp(&p, &orig, sizeof p);
            printf("%d\n", (int)ok);
        } else if (op[0] == 'A') {  // A X Y Z: to_affine, and the blst_p2 conversions there and back
            g2::Jac p;
            if (!rd2(p.x) || !rd2(p.y) || !rd2(p.z)) return 2;
            g2::AffPt a;
            g2::to_affine(a, p);
            const hp::G2Affine want = hp::g2_to_affine(specj(p));
            raw2(a.x); raw2(a.y);
            bool ok = (a.flags & 1) == (want.inf ? 1u : 0u) && hp::f2_eq(spec(a.x), want.x) && hp::f2_eq(spec(a.y), want.y);
            const hp::G2Jac j = specj(p);
            g2::Jac back;
            g2::from_blst_jacobian(back, reinterpret_cast<const ff::Fp*>(&j));
            ok = ok && same(specj(back), j) && g2::is_inf(back) == hp::g2_is_inf(j);
            printf("%u %d\n", a.flags, (int)ok);
        } else return 4;
    }
    return 0;
}
'''


def limbs(v):
    assert 0 <= v < 1 << 392
    return [(v >> (28 * i)) & M28 for i in range(13)] + [v >> 364]


def value(l):
    return sum(x << (28 * i) for i, x in enumerate(l))


def rep(v, k):
    """the Montgomery residue of the field element v plus k * p"""
    return v * R392 % P + k * P


def fe(v):
    return " ".join("%x" % x for x in limbs(v))


# ---- Fp2 on Python integers: pairs (c0, c1), u^2 = -1
def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], P - 2, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2mul(r, a)
        a = f2mul(a, a)
        e >>= 1
    return r


def f2sqrt(a):
    """p = 3 mod 4 (Adj, Rodriguez-Henriquez, algorithm 9); None when a is no square"""
    if a == (0, 0):
        return a
    a1 = f2pow(a, (P - 3) // 4)
    alpha = f2mul(f2mul(a1, a1), a)
    x0 = f2mul(a1, a)
    if alpha == (P - 1, 0):
        x = (-x0[1] % P, x0[0])
    else:
        x = f2mul(f2pow(f2add((1, 0), alpha), (P - 1) // 2), x0)
    return x if f2mul(x, x) == a else None


def twist_point(rnd):
    while True:
        x = (rnd.randrange(P), rnd.randrange(P))
        y = f2sqrt(f2add(f2mul(f2mul(x, x), x), (4, 4)))
        if y is not None and y != (0, 0):
            return x, (y if rnd.random() < 0.5 else f2sub((0, 0), y))


def aff_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if a[1] != b[1] or a[1] == (0, 0):
            return None
        lam = f2mul(f2mul((3, 0), f2mul(a[0], a[0])), f2inv(f2add(a[1], a[1])))
    else:
        lam = f2mul(f2sub(b[1], a[1]), f2inv(f2sub(b[0], a[0])))
    x3 = f2sub(f2sub(f2mul(lam, lam), a[0]), b[0])
    return x3, f2sub(f2mul(lam, f2sub(a[0], x3)), a[1])


class Script:
    def __init__(self):
        self.lines, self.checks = [], []

    def f2(self, name, a, b, bounds, want=None):
        """a, b: pairs of representative integers; bounds: (c0, c1) multiples of p the output stays below"""
        self.lines.append("F%s %s %s %s %s" % (name, fe(a[0]), fe(a[1]), fe(b[0]), fe(b[1])))
        self.checks.append(("F" + name, bounds, want))

    def jac(self, aff, z, ks):
        """representatives of the Jacobian point over the affine point aff with this Z, plus ks multiples of p (six)"""
        z2 = f2mul(z, z)
        x, y = f2mul(aff[0], z2), f2mul(aff[1], f2mul(z2, z))
        return [rep(c, k) for c, k in zip(x + y + z, ks)]

    def dbl(self, comps, want):
        self.lines.append("D " + " ".join(fe(c) for c in comps))
        self.checks.append(("D", (2, 2, 2, 2, 10, 10), want))

    def madd(self, comps, pt, state, want, tag):
        self.lines.append("M " + " ".join(fe(c) for c in comps) + " " + " ".join(fe(c) for c in pt))
        self.checks.append(("M " + tag, (3, 3, 3, 3, 10, 10), (state, want)))

    def tab(self, comps, pt, flags, neg, want, tag):
        self.lines.append("T " + " ".join(fe(c) for c in comps) + " " + " ".join(fe(c) for c in pt) + " %x %x" % (flags, neg))
        self.checks.append(("T " + tag, (3, 3, 3, 3, 10, 10), (flags, want)))

    def aff(self, comps, want):
        self.lines.append("A " + " ".join(fe(c) for c in comps))
        self.checks.append(("A", (1, 1, 1, 1), want))


def pattern_values(bound):
    """representatives below bound * p whose limbs 0..12 are all ones / all zero"""
    top_max = (bound * P) >> 364
    out = []
    for low in (LOW_ONES, 0):
        for top in (0, 1, top_max - 1):
            v = (top << 364) | low
            if v < bound * P:
                out.append(v)
    return out


def build_script(rnd):
    s = Script()
    rv = lambda bound: rep(rnd.randrange(P), rnd.randrange(bound))
    top = lambda bound: rep(rnd.randrange(P), bound - 1)
    # ---- Fp2 routines: (name, bound of a, bound of b, output bounds)
    table = [("add", 32, 31, (63, 63)), ("dbl", 31, 1, (62, 62)), ("sub4", 10, 3, (14, 14)), ("sub8", 10, 7, (18, 18)),
             ("sub16", 10, 15, (26, 26)), ("sub32", 16, 31, (48, 48)), ("neg2", 1, 1, (3, 3)), ("neg16", 15, 1, (17, 17)),
             ("mul", 21, 30, (6, 10)), ("mul", 63, 10, (6, 10)), ("mul", 25, 25, (6, 10)), ("sqr", 15, 1, (2, 4)),
             ("mulfe", 63, 40, (2, 2)), ("red", 63, 1, (2, 2)), ("inv", 15, 1, (2, 2)), ("iszero", 63, 1, None)]
    for name, ba, bb, ob in table:
        for it in range(24):
            pick = (rv, top)[it & 1]
            s.f2(name, (pick(ba), pick(ba)), (pick(bb), pick(bb)), ob)
        pa, pb = pattern_values(ba), pattern_values(bb)
        for va in pa:
            for vb in pb[:3]:
                if name == "inv" and va % P == 0:
                    continue
                s.f2(name, (va, pa[0]), (vb, pb[-1]), ob)
                s.f2(name, (pa[-1], va), (pb[0], vb), ob)
    # exact zero tests: multiples of p on both components, on one, and one off
    for k0 in (0, 1, 13, 62):
        for k1 in (0, 5, 62):
            s.f2("iszero", (k0 * P, k1 * P), (0, 0), None, want=1)
            s.f2("iszero", (k0 * P + 1, k1 * P), (0, 0), None, want=0)
            s.f2("iszero", (k0 * P, k1 * P + (1 << 364)), (0, 0), None, want=0)
    # ---- points
    for it in range(40):
        a, b = twist_point(rnd), twist_point(rnd)
        z = (rnd.randrange(P), rnd.randrange(P))
        hi = it & 1
        # doubling over its input bounds X, Y < 15, Z < 21
        ks = [14, 14, 14, 14, 20, 20] if hi else [rnd.randrange(15) for _ in range(4)] + [rnd.randrange(21), rnd.randrange(21)]
        s.dbl(s.jac(a, z, ks), aff_add(a, a))
        # additions over X1, Y1 < 3, Z1 < 10, table point x, y < 3
        ks = [2, 2, 2, 2, 9, 9] if hi else [rnd.randrange(3) for _ in range(4)] + [rnd.randrange(10), rnd.randrange(10)]
        kp = [2] * 4 if hi else [rnd.randrange(3) for _ in range(4)]
        pt = lambda q: [rep(c, k) for c, k in zip(q[0] + q[1], kp)]
        nb = (b[0], f2sub((0, 0), b[1]))
        s.madd(s.jac(a, z, ks), pt(b), DONE, aff_add(a, b), "random")
        s.madd(s.jac(b, z, ks), pt(b), DOUBLE, aff_add(b, b), "P + P")
        s.madd(s.jac(b, z, ks), pt(nb), INF, None, "P - P")
        s.madd([0] * 6, pt(b), DONE, b, "infinity + P")
        other = (b[0], f2add(b[1], (1 + it, it)))  # equal x, another y (not on the curve: the formulas give infinity)
        s.madd(s.jac(b, z, ks), pt(other), INF, None, "equal x, other y")
        s.madd(s.jac(a, (1, 0), [0] * 6), pt(b), DONE, aff_add(a, b), "Z = 1")
        s.aff(s.jac(a, z, [14] * 6 if hi else [rnd.randrange(15) for _ in range(6)]), a)
        # the table step: canonical entries, both signs, the flag
        can = lambda q: [rep(c, 0) for c in q[0] + q[1]]
        s.tab(s.jac(a, z, ks), can(b), 0, 0, aff_add(a, b), "plus")
        s.tab(s.jac(a, z, ks), can(b), 0, 1, aff_add(a, nb), "minus")
        s.tab(s.jac(a, z, ks), can(b), 1, it & 1, a, "infinite entry")
        s.tab([0] * 6, can(b), 1, it & 1, None, "infinite entry onto infinity")
        s.tab([0] * 6, can(b), 0, 1, nb, "infinity minus P")
        s.tab(s.jac(b, z, ks), can(b), 0, 0, aff_add(b, b), "P + P")
        s.tab(s.jac(b, z, ks), can(b), 0, 1, None, "P - P")
        s.tab(s.jac(nb, z, ks), can(b), 0, 1, aff_add(nb, nb), "-P - P")
    s.aff([0] * 6, None)
    # limb patterns inside a point: Y1 and Z1 with limbs 0..12 all ones / all zero under a small top limb
    for low in (LOW_ONES, 0):
        for topl in (1, 0x1a011, 0x34021):
            a, b = twist_point(rnd), twist_point(rnd)
            v = (topl << 364) | low
            zc = (v * pow(R392, -1, P) % P, rnd.randrange(P))
            comps = s.jac(a, zc, [0] * 6)
            comps[4] = v
            s.madd(comps, [rep(c, 0) for c in b[0] + b[1]], DONE, aff_add(a, b), "pattern Z")
            s.dbl(comps, aff_add(a, a))
    return s


def compile_program(tmp_path, name, extra):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / (name + ".cpp")
    src.write_text(PROGRAM)
    exe = tmp_path / name
    cmd = [cxx, "-O1", "-std=c++17"] + extra + ["-I", CSRC, str(src), "-o", str(exe), "-lpthread"]
    return cmd, exe


def run_and_check(exe, s):
    run = subprocess.run([str(exe)], input="\n".join(s.lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    out = run.stdout.strip().split("\n")
    assert len(out) == len(s.checks) > 1000
    seen = set()
    for (tag, bounds, want), ln in zip(s.checks, out):
        t = [int(x, 16) for x in ln.split()]
        assert t[-1] == 1, "%s: differs from host_pairing.h" % tag
        if tag == "Fiszero":
            if want is not None:
                assert t[0] == want, tag
            continue
        body = t[1:-1] if tag[0] in "MT" else t[:-2] if tag == "A" else t[:-1]
        comps = [body[14 * k:14 * k + 14] for k in range(len(body) // 14)]
        assert len(comps) == len(bounds), tag
        if tag[0] == "M":
            state, aff = want
            assert t[0] == state, "%s: state %d, expected %d" % (tag, t[0], state)
            seen.add((tag, state))
        if tag == "A":
            assert t[-2] == (1 if want is None else 0), tag
        if tag[0] == "T":
            assert t[0] == want[0], tag
            seen.add((tag, want[1] is None))
        inf = tag[0] in "MDT" and all(x == 0 for c in comps[4:6] for x in c)
        for c, b in zip(comps, bounds):
            assert all(x <= M28 for x in c[:13]), "%s: not normalized" % tag
            assert value(c) < b * P or (tag == "Fneg2" and value(c) <= 2 * P), "%s: %d p and more" % (tag, value(c) // P)
        # the result as field elements, against the chord / tangent formulas on Python integers
        if tag[0] in "MDT":
            aff = want[1] if tag[0] in "MT" else want
            assert inf == (aff is None), tag
            if aff is not None:
                rinv = pow(R392, -1, P)
                v = [value(c) * rinv % P for c in comps]
                zi = f2inv((v[4], v[5]))
                zi2 = f2mul(zi, zi)
                assert (f2mul((v[0], v[1]), zi2), f2mul((v[2], v[3]), f2mul(zi2, zi))) == aff, "%s: not the group law's answer" % tag
        if tag == "A" and want is not None:
            rinv = pow(R392, -1, P)
            assert all(value(c) < P for c in comps), "to_affine is canonical"
            v = [value(c) * rinv % P for c in comps]
            assert ((v[0], v[1]), (v[2], v[3])) == want, tag
    for need in (("T infinite entry", False), ("T infinite entry onto infinity", True), ("T P + P", False), ("T P - P", True),
                 ("T -P - P", False), ("T infinity minus P", False)):
        assert need in seen, need
    for need in (("M P + P", DOUBLE), ("M P - P", INF), ("M infinity + P", DONE), ("M equal x, other y", INF), ("M random", DONE)):
        assert need in seen, need


@pytest.mark.parametrize("exact", [False, True])
def test_fp2_and_g2_lane_arithmetic_against_the_host_specification(tmp_path, exact):
    s = build_script(random.Random(0x62))
    cmd, exe = compile_program(tmp_path, "g2check", ["-DKZGAMD_FORCE_EXACT_TESTS"] if exact else [])
    subprocess.check_call(cmd)
    run_and_check(exe, s)


def test_no_undefined_behaviour_in_the_lane_arithmetic(tmp_path):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("g++")
    flags = ["-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([cxx, "-O1", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (probed.stderr.strip().split("\n") or [""])[-1])
    cmd, exe = compile_program(tmp_path, "g2check_ubsan", flags)
    cmd[0] = cxx
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    s = build_script(random.Random(0x62))
    run = subprocess.run([str(exe)], input="\n".join(s.lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and "runtime error" not in run.stderr, run.stderr[-2000:]
    assert len(run.stdout.strip().split("\n")) == len(s.checks)


def test_groupmul_cross_compiles_for_gfx950_with_the_products_flags(tmp_path):
    spec = importlib.util.spec_from_file_location("rust_kzg_amd_build_g2", os.path.join(ROOT, "rust-kzg_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "groupmul.hip" in b.SOURCES and "g2_28.hip.h" in b.HEADERS
    out = str(tmp_path / "groupmul.o")
    p = subprocess.run([b.hipcc_path()] + b.COMPILE_FLAGS + ["-fPIC", "-c", os.path.join(CSRC, "groupmul.hip"), "-o", out],
                       capture_output=True, text=True)
    assert p.returncode == 0 and os.path.getsize(out) > 0, p.stderr[-3000:]
