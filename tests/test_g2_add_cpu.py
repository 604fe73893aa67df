"""g2::add (g2_28.hip.h: the complete addition of two Jacobian G2 points) and the lane's walk of a G2 linear
combination (g2_lincomb.hip.h), compiled for the host and held to host_pairing.h, the specification, in the manner of
tests/test_g2_lane_cpu.py: canonical residues compared inside one stand-alone program, output bounds checked here against
the header's table (X, Y < 2, Z < 10), and the sum as a group element against the chord / tangent formulas on Python
integers.  Both flavours of the exact zero test.

Inputs of g2::add:
  random    pairs of curve points of E'(Fp2), random Z on both sides, representatives spread over X, Y < 3, Z < 10;
  top       every component at the top of those bounds (2p and 9p added to a residue);
  infinity  either operand, and both;
  P + P     the same point under two different Z (the doubling of g2_add), P + (-P) (infinity);
  Z = 1     on one side, and on both;
  order 13  a point of order 13 of the twist (tests/g2_encodings.py has it): T + T, T + 12 T = infinity, 6 T + 7 T;
  fed back  K: from P, Q and an affine R the three outputs dbl(P), madd(P, R), add(P, Q), inputs at the top of their
            bounds, then add of every ordered pair of them, dbl of each and madd of each: the output of any of the
            three routines as an input of any of them.
The walk: W runs g2lc::term for every scalar of setup_model.scalar_cases() (872) over a handful of points (generator
multiples with Z != 1, the order-13 point, an identity), sums them 64 at a time with g2lc::tree_step level by level as
k_g2_lincomb_terms does, sums the partial sums the same way as k_g2_sum does, and compares with pairing::g2_mul followed
by g2_add."""
import importlib.util
import os
import random
import shutil
import subprocess

import pytest

import codec_model as CM
import setup_model as S
from test_g2_lane_cpu import CSRC, P, ROOT, M28, R392, aff_add, f2inv, f2mul, f2sub, fe, rep, twist_point, value

PROGRAM = r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "g2_28.hip.h"
#include "g2_lincomb.hip.h"
#include "host_pairing.h"
namespace hp = kzgamd::pairing;
using fp28::Fe;
using g2::F2;
static bool rd(Fe& r) { for (int i = 0; i < 14; ++i) if (scanf("%x", &r.v[i]) != 1) return false; return true; }
static bool rd2(F2& r) { return rd(r.c0) && rd(r.c1); }
static bool rdj(g2::Jac& p) { return rd2(p.x) && rd2(p.y) && rd2(p.z); }
static void raw(const Fe& a) { for (int i = 0; i < 14; ++i) printf("%x ", a.v[i]); }
static void raw2(const F2& a) { raw(a.c0); raw(a.c1); }
static void rawj(const g2::Jac& p) { raw2(p.x); raw2(p.y); raw2(p.z); }
static hp::Fp2 spec(const F2& a) { ff::Fp o[2]; g2::to_blst(o, a); return {o[0], o[1]}; }
static hp::G2Jac specj(const g2::Jac& p) { hp::G2Jac r; g2::to_blst_jacobian(reinterpret_cast<ff::Fp*>(&r), p); return r; }
static bool same(const hp::G2Jac& a, const hp::G2Jac& b) { return hp::f2_eq(a.x, b.x) && hp::f2_eq(a.y, b.y) && hp::f2_eq(a.z, b.z); }
static bool add_ok(const g2::Jac& p, const g2::Jac& q, g2::Jac& out) {
    out = p;
    g2::add(out, q);
    return same(specj(out), hp::g2_add(specj(p), specj(q)));
}
// the 64 slots summed into slot 0, level by level as the kernels' tree_sum does
static void tree(g2::Jac* slots) {
    for (int half = g2lc::LANES / 2; half >= 1; half >>= 1)
        for (int t = 0; t < half; ++t) g2lc::tree_step(slots, t, half);
}
static g2::Jac sum_all(std::vector<g2::Jac> v) {  // k_g2_sum, launch after launch
    while (true) {
        std::vector<g2::Jac> next;
        for (size_t at = 0; at < v.size(); at += g2lc::LANES) {
            g2::Jac slots[g2lc::LANES];
            for (int t = 0; t < g2lc::LANES; ++t) {
                if (at + t < v.size()) slots[t] = v[at + t];
                else g2::set_inf(slots[t]);
            }
            tree(slots);
            next.push_back(slots[0]);
        }
        if (next.size() == 1) return next[0];
        v.swap(next);
    }
}
int main() {
    char op[16];
    while (scanf("%15s", op) == 1) {
        if (op[0] == 'S') {  // S P Q
            g2::Jac p, q, r;
            if (!rdj(p) || !rdj(q)) return 2;
            const bool ok = add_ok(p, q, r);
            rawj(r);
            printf("%d\n", (int)ok);
        } else if (op[0] == 'K') {  // K P Q x2 y2: outputs of dbl, madd, add fed back into each
            g2::Jac p, q, o[3], r;
            F2 x2, y2;
            if (!rdj(p) || !rdj(q) || !rd2(x2) || !rd2(y2)) return 2;
            o[0] = p; g2::dbl(o[0]);
            o[1] = p; g2::madd_complete(o[1], x2, y2);
            bool ok = add_ok(p, q, o[2]);
            const hp::G2Jac aff = {spec(x2), spec(y2), hp::f2_one()};
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) {
                    ok = add_ok(o[i], o[j], r) && ok;
                    rawj(r);
                }
                r = o[i]; g2::dbl(r);
                ok = same(specj(r), hp::g2_dbl(specj(o[i]))) && ok;
                r = o[i]; g2::madd_complete(r, x2, y2);
                ok = same(specj(r), hp::g2_add(specj(o[i]), aff)) && ok;
            }
            printf("%d\n", (int)ok);
        } else if (op[0] == 'W') {  // W npoints nterms, the points, then (point index, 8 scalar words) per term
            int np, nt;
            if (scanf("%d %d", &np, &nt) != 2) return 2;
            std::vector<hp::G2Jac> pts(np);
            for (auto& p : pts) { g2::Jac j; if (!rdj(j)) return 2; p = specj(j); }
            std::vector<g2::Jac> terms(nt);
            hp::G2Jac want = hp::g2_inf();
            std::vector<g2::Jac> part;
            for (int i = 0; i < nt; ++i) {
                int at;
                ff::Fr k;
                if (scanf("%d", &at) != 1) return 2;
                for (int w = 0; w < 8; ++w) if (scanf("%x", &k.v[w]) != 1) return 2;
                g2lc::term(terms[i], reinterpret_cast<const ff::Fp*>(&pts[at]), ff::to_mont(k));
                want = hp::g2_add(want, hp::g2_mul(pts[at], k.v));
            }
            for (int at = 0; at < nt; at += g2lc::LANES) {  // k_g2_lincomb_terms: a workgroup's 64 terms
                g2::Jac slots[g2lc::LANES];
                for (int t = 0; t < g2lc::LANES; ++t) {
                    if (at + t < nt) slots[t] = terms[at + t];
                    else g2::set_inf(slots[t]);
                }
                tree(slots);
                part.push_back(slots[0]);
            }
            const g2::Jac got = sum_all(part);
            rawj(got);
            printf("%d\n", (int)hp::g2_equal(specj(got), want) && (hp::g2_is_inf(want) == g2::is_inf(got)));
        } else return 4;
    }
    return 0;
}
'''


def jac(aff, z, ks):
    """representatives of the Jacobian point over aff with this Z plus ks multiples of p (six); None: infinity"""
    if aff is None:
        return [0] * 6
    z2 = f2mul(z, z)
    x, y = f2mul(aff[0], z2), f2mul(aff[1], f2mul(z2, z))
    return [rep(c, k) for c, k in zip(x + y + z, ks)]


def neg(a):
    return None if a is None else (a[0], f2sub((0, 0), a[1]))


def mul(k, a):
    r = None
    while k:
        if k & 1:
            r = aff_add(r, a)
        a = aff_add(a, a)
        k >>= 1
    return r


TOP = [2, 2, 2, 2, 9, 9]


class Script:
    def __init__(self):
        self.lines, self.checks = [], []

    def add(self, p, q, want, tag):
        self.lines.append("S " + " ".join(fe(c) for c in p + q))
        self.checks.append(("S " + tag, 1, want))

    def fed_back(self, p, q, pt):
        self.lines.append("K " + " ".join(fe(c) for c in p + q + pt))
        self.checks.append(("K", 9, None))

    def walk(self, points, terms, tag):
        body = ["W %d %d" % (len(points), len(terms))] + [" ".join(fe(c) for c in p) for p in points]
        body += ["%d %s" % (at, " ".join("%x" % ((k >> (32 * w)) & 0xffffffff) for w in range(8))) for at, k in terms]
        self.lines.append("\n".join(body))
        self.checks.append(("W " + tag, 1, None))


def build_script(rnd):
    s = Script()
    rz = lambda: (rnd.randrange(P), rnd.randrange(P))
    rk = lambda: [rnd.randrange(3) for _ in range(4)] + [rnd.randrange(10), rnd.randrange(10)]
    one = (1, 0)
    for it in range(24):
        a, b = twist_point(rnd), twist_point(rnd)
        ks = (lambda: TOP) if it & 1 else rk
        s.add(jac(a, rz(), ks()), jac(b, rz(), ks()), aff_add(a, b), "random")
        s.add(jac(a, rz(), ks()), jac(a, rz(), ks()), aff_add(a, a), "P + P")
        s.add(jac(a, rz(), ks()), jac(neg(a), rz(), ks()), None, "P - P")
        s.add(jac(None, None, None), jac(b, rz(), ks()), b, "infinity + Q")
        s.add(jac(a, rz(), ks()), jac(None, None, None), a, "P + infinity")
        s.add(jac(a, one, [0] * 6), jac(b, rz(), ks()), aff_add(a, b), "Z1 = 1")
        s.add(jac(a, rz(), ks()), jac(b, one, [0] * 6), aff_add(a, b), "Z2 = 1")
        s.add(jac(a, one, [0] * 6), jac(b, one, [0] * 6), aff_add(a, b), "Z1 = Z2 = 1")
        s.add(jac(a, one, [0] * 6), jac(a, one, [0] * 6), aff_add(a, a), "P + P, Z = 1")
        pt = [rep(c, 2 if it & 1 else rnd.randrange(3)) for c in b[0] + b[1]]
        s.fed_back(jac(a, rz(), ks()), jac(b, rz(), ks()), pt)
        s.fed_back(jac(b, rz(), ks()), jac(b, rz(), ks()), pt)  # P = Q = R: doublings everywhere
    s.add(jac(None, None, None), jac(None, None, None), None, "infinity + infinity")
    t = CM.torsion_point(13)
    assert mul(13, t) is None and mul(12, t) == neg(t)
    for ks in (TOP, [0] * 6):
        s.add(jac(t, rz(), ks), jac(t, rz(), ks), mul(2, t), "order 13: T + T")
        s.add(jac(t, rz(), ks), jac(mul(12, t), rz(), ks), None, "order 13: T + 12 T")
        s.add(jac(mul(6, t), rz(), ks), jac(mul(7, t), rz(), ks), None, "order 13: 6 T + 7 T")
        s.add(jac(mul(5, t), rz(), ks), jac(mul(6, t), rz(), ks), mul(11, t), "order 13: 5 T + 6 T")
    # ---- the walk
    g = CM.G2
    points = [jac(g, one, [0] * 6), jac(mul(7, g), rz(), [0] * 6), jac(mul(12, g), rz(), [0] * 6), jac(t, rz(), [0] * 6),
              jac(None, None, None), jac(twist_point(rnd), rz(), [0] * 6)]
    cases = S.scalar_cases()
    assert len(cases) == 872
    s.walk(points, [(i % 3, k) for i, k in enumerate(cases)], "every scalar case over three subgroup points")
    s.walk(points, [(3 + i % 3, k) for i, k in enumerate(cases[:200])], "order 13, the identity and a point of full order")
    s.walk(points, [(1, k) for k in cases[6:6 + 65]] + [(1, S.R - k) for k in cases[6:6 + 65]], "k P and (r - k) P: the identity")
    s.walk(points, [(1, 5)] * 130, "equal terms: every tree addition a doubling")
    s.walk(points, [(4, 5), (0, 0)], "nothing but identities")
    s.walk(points, [(2, cases[9])], "one term")
    return s


def compile_program(tmp_path, name, extra):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / (name + ".cpp")
    src.write_text(PROGRAM)
    exe = tmp_path / name
    return [cxx, "-O2", "-std=c++17"] + extra + ["-I", CSRC, str(src), "-o", str(exe), "-lpthread"], exe


def run_and_check(exe, s):
    run = subprocess.run([str(exe)], input="\n".join(s.lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    out = run.stdout.strip().split("\n")
    assert len(out) == len(s.checks) > 250
    rinv = pow(R392, -1, P)
    seen = set()
    for (tag, npts, want), ln in zip(s.checks, out):
        t = [int(x, 16) for x in ln.split()]
        assert t[-1] == 1, "%s: differs from host_pairing.h" % tag
        assert len(t) == 1 + npts * 84, tag
        for k in range(npts):
            comps = [t[84 * k + 14 * c:84 * k + 14 * c + 14] for c in range(6)]
            inf = all(x == 0 for c in comps[4:6] for x in c)
            if inf:
                assert all(x == 0 for c in comps for x in c), "%s: the identity is all-zero" % tag
            for c, b in zip(comps, (3, 3, 3, 3, 10, 10) if inf or tag[0] == "W" else (2, 2, 2, 2, 10, 10)):
                # a sum that came back as one operand (the other at infinity) keeps that operand's bounds: X, Y < 3
                b = 3 if tag in ("S infinity + Q", "S P + infinity") and b == 2 else b
                assert all(x <= M28 for x in c[:13]), "%s: not normalized" % tag
                assert value(c) < b * P, "%s: %d p and more" % (tag, value(c) // P)
            if tag[0] == "S":
                assert inf == (want is None), tag
                seen.add((tag, inf))
                if want is not None:
                    v = [value(c) * rinv % P for c in comps]
                    zi = f2inv((v[4], v[5]))
                    zi2 = f2mul(zi, zi)
                    assert (f2mul((v[0], v[1]), zi2), f2mul((v[2], v[3]), f2mul(zi2, zi))) == want, "%s: not the group law's answer" % tag
            if tag in ("W k P and (r - k) P: the identity", "W nothing but identities"):
                assert inf, tag
    for need in (("S P + P", False), ("S P - P", True), ("S infinity + Q", False), ("S P + infinity", False), ("S infinity + infinity", True),
                 ("S order 13: T + 12 T", True), ("S order 13: T + T", False), ("S Z1 = Z2 = 1", False)):
        assert need in seen, need


@pytest.mark.parametrize("exact", [False, True])
def test_g2_add_and_the_lincomb_walk_against_the_host_specification(tmp_path, exact):
    s = build_script(random.Random(0x6a))
    cmd, exe = compile_program(tmp_path, "g2add", ["-DKZGAMD_FORCE_EXACT_TESTS"] if exact else [])
    subprocess.check_call(cmd)
    run_and_check(exe, s)


def test_no_undefined_behaviour_in_g2_add_and_the_walk(tmp_path):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("g++")
    flags = ["-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([cxx, "-O1", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (probed.stderr.strip().split("\n") or [""])[-1])
    cmd, exe = compile_program(tmp_path, "g2add_ubsan", flags)
    cmd[0] = cxx
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    s = build_script(random.Random(0x6a))
    run = subprocess.run([str(exe)], input="\n".join(s.lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and "runtime error" not in run.stderr, run.stderr[-2000:]
    assert len(run.stdout.strip().split("\n")) == len(s.checks)


def test_setupcheck_cross_compiles_for_gfx950_with_the_products_flags(tmp_path):
    spec = importlib.util.spec_from_file_location("rust_kzg_amd_build_g2add", os.path.join(ROOT, "rust-kzg_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "setupcheck.hip" in b.SOURCES and "g2_lincomb.hip.h" in b.HEADERS and "setupcheck_internal.h" in b.HEADERS
    out = str(tmp_path / "setupcheck.o")
    p = subprocess.run([b.hipcc_path()] + b.COMPILE_FLAGS + ["-fPIC", "-c", os.path.join(CSRC, "setupcheck.hip"), "-o", out],
                       capture_output=True, text=True)
    assert p.returncode == 0 and os.path.getsize(out) > 0, p.stderr[-3000:]
