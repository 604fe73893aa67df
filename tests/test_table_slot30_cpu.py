"""The wide table's slot in the limbs of the accumulation chain (g1s::WidePt30), the chain_add overload that takes such a
slot's coordinates, and the way back with psi in its constants (g1s::to_xyzz28 with a `part`) — compiled for the host
from the headers alone, with -fsanitize=undefined,address, and held to Python integers.

  slot       pack_slot(X, Y, flags) holds fp30s::from28 of the canonical values limb for limb, fp30s::to28 and
             fp30s::to28_unsigned give them back limb for limb, and the flag word (word 26) and the zero padding survive a trip through memory;
  chain_add  the overload over fp30s::Fe and the one over fp28::Fe leave identical accumulator limbs over a chain of 64
             table points with both signs, an equal pair and an opposite pair;
  way back   to_xyzz28 with a part equals, limb for limb after fp28::canon, the plain to_xyzz28 followed by the two fp28
             products it replaces (x * beta28(), neg<8>(y) * one()), for both parts on the states empty, single point
             and sum; what it stores is normalized and inside the interval the header documents;
  constant   4 * beta * 2^390 mod p, read from the header, against beta28() of msm.hip and k4 as Python integers;
  model      the constant and the negated Y through the bounds propagation of fp30s_model.py."""
import os
import random
import re
import shutil
import subprocess
from fractions import Fraction as Fr

import pytest

import fp30s_model as M
from test_madd_forms_cpu import EMPTY, AFFINE, XYZZ, P, affine_add, curve_point, limbs as limbs28, mont as mont28, neg, value as value28

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-kzg_amd", "csrc")
R392 = 1 << 392
R392INV = pow(R392, -1, P)

PROGRAM = r'''
#include <cstdio>
#include <cstring>
#include "g1_30s.hip.h"
using fp30s::Fe;
static fp28::Fe rd28() { fp28::Fe r; for (int i = 0; i < 14; ++i) if (scanf("%x", &r.v[i]) != 1) r.v[i] = 0; return r; }
static void raw(const Fe& a) { for (int i = 0; i < 13; ++i) printf("%d ", a.v[i]); }
static void raw28(const fp28::Fe& a) { for (int i = 0; i < 14; ++i) printf("%x ", a.v[i]); }
static void raw4(const g1s::Xyzz& a) { raw(a.x); raw(a.y); raw(a.zzz); raw(a.zz); }
static void raw4(const g1::Xyzz& a) { raw28(a.x); raw28(a.y); raw28(a.zzz); raw28(a.zz); }
static g1::Xyzz canon4(const g1::Xyzz& a) { g1::Xyzz r; r.x = fp28::canon(a.x); r.y = fp28::canon(a.y); r.zzz = fp28::canon(a.zzz); r.zz = fp28::canon(a.zz); return r; }
int main() {
    const fp30s::Seeds sd = fp30s::seeds();
    char op[16];
    g1s::Xyzz a_old, a_new;
    g1s::set_inf(a_old);
    g1s::set_inf(a_new);
    ff::u32 st_old = g1::CHAIN_EMPTY, st_new = g1::CHAIN_EMPTY;
    fp28::Fe beta = fp28::zero();
    while (scanf("%15s", op) == 1) {
        if (!strcmp(op, "slot")) {  // flags x y -> the 32 words of the slot as they lie in memory; from28; to28 of the unpacked slot
            unsigned flags;
            if (scanf("%u", &flags) != 1) return 1;
            const fp28::Fe x = rd28(), y = rd28();
            const g1s::WidePt30 s = g1s::pack_slot(x, y, flags);
            alignas(128) unsigned char mem[128];
            memcpy(mem, &s, 128);
            ff::u32 w[32];
            memcpy(w, mem, 128);
            for (int i = 0; i < 32; ++i) printf("%u ", w[i]);
            g1s::WidePt30 back;
            memcpy(&back, mem, 128);
            raw(fp30s::from28(x)); raw(fp30s::from28(y));
            raw28(fp30s::to28(back.x)); raw28(fp30s::to28(back.y));
            raw28(fp30s::to28_unsigned(back.x)); raw28(fp30s::to28_unsigned(back.y));
            printf("%u ", back.flags);
            for (int i = 0; i < 5; ++i) printf("%u ", back.pad[i]);
        } else if (!strcmp(op, "beta")) {
            beta = rd28();
            printf("ok");
        } else if (!strcmp(op, "reset")) {
            g1s::set_inf(a_old); g1s::set_inf(a_new); st_old = st_new = g1::CHAIN_EMPTY;
            printf("ok");
        } else if (!strcmp(op, "add")) {  // m x y: the overload over fp28 limbs on one accumulator, the one over a slot on the other
            unsigned m;
            if (scanf("%u", &m) != 1) return 1;
            const fp28::Fe x = rd28(), y = rd28();
            const g1s::WidePt30 s = g1s::pack_slot(x, y, 0);
            g1s::chain_add(a_old, st_old, x, y, m ? 0xffffffffu : 0u, sd);
            g1s::chain_add(a_new, st_new, s.x, s.y, m ? 0xffffffffu : 0u, sd);
            printf("%u %u ", st_old, st_new);
            raw4(a_old); raw4(a_new);
        } else if (!strcmp(op, "fin")) {  // part: what k_fbw_accum stored before, canonical; the new form, canonical; the new form as stored
            unsigned part;
            if (scanf("%u", &part) != 1) return 1;
            g1::Xyzz o, n;
            g1s::to_xyzz28(o, a_old, st_old, sd);
            if (part && st_old != g1::CHAIN_EMPTY) {
                o.x = fp28::mul(o.x, beta);
                o.y = fp28::mul(fp28::neg<8>(o.y), fp28::one());
            }
            g1s::to_xyzz28(n, a_new, st_new, part, sd);
            printf("%u ", st_new);
            raw4(canon4(o)); raw4(canon4(n)); raw4(n);
        } else return 1;
        printf("\n");
    }
    printf("done\n");
    return 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """the program with both sanitizers; without them only where their runtime is not installed (decided on an empty
    program with the same flags) — every failure to build the real program fails"""
    tmp = tmp_path_factory.mktemp("slot30")
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    san = ["-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([cxx] + san + [str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp / "probe")]).returncode != 0:
        print("no sanitizer runtime, building without: " + (probed.stderr.strip().split("\n") or [""])[-1])
        san = []
    src = tmp / "slot30_check.cpp"
    src.write_text(PROGRAM)
    out = tmp / "slot30_check"
    built = subprocess.run([cxx, "-O1", "-std=c++17"] + san + ["-I", CSRC, str(src), "-o", str(out)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return out


def run(exe, lines):
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.strip().split("\n")
    assert out[-1] == "done" and len(out) == len(lines) + 1
    return out[:-1]


def fmt28(l):
    return " ".join("%x" % v for v in l)


def header_constant(name):
    text = open(os.path.join(CSRC, "g1_30s.hip.h")).read()
    found = set(re.findall(r"constexpr i32 %s\[L\] = \{([^}]*)\}" % name, text))
    assert len(found) == 1, name  # one value, however many times the header states it
    l = [int(v, 16) for v in found.pop().replace(" ", "").replace("\n", "").split(",")]
    assert len(l) == 13
    return l


def beta28_limbs():
    text = open(os.path.join(CSRC, "msm.hip")).read()
    m = re.search(r"fp28::Fe beta28\(\) \{\s*constexpr u32 t\[14\] = \{([^}]*)\}", text)
    l = [int(v.strip().rstrip("u"), 16) for v in m.group(1).split(",")]
    assert len(l) == 14
    return l


def slot_values():
    rnd = random.Random(0x51070)
    vals = [0, 1, P - 1]
    for k in range(1, 13):
        vals += [(1 << (30 * k)) - 1, 1 << (30 * k), (1 << (30 * k)) + 1]
    for j in range(1, 14):
        vals += [(1 << (28 * j)) - 1, (1 << (28 * j)) + 1]
    assert all(0 <= v < P for v in vals)
    return vals + [rnd.randrange(P) for _ in range(100000)]


def test_slot_is_from28_and_to28_gives_it_back(exe):
    vals = slot_values()
    n = len(vals)
    assert n == 3 + 36 + 26 + 100000
    flags = [(0, 1, 0xffffffff, 0x80000000)[k % 4] if k % 7 == 0 else 0 for k in range(n)]
    lines = ["slot %u %s %s" % (flags[k], fmt28(limbs28(vals[k])), fmt28(limbs28(vals[n - 1 - k]))) for k in range(n)]
    for k, ln in enumerate(run(exe, lines)):
        t = ln.split()
        x, y = vals[k], vals[n - 1 - k]
        w = [int(v) for v in t[:32]]
        f28 = [int(v) for v in t[32:58]]
        b28 = [int(v, 16) for v in t[58:86]]
        u28 = [int(v, 16) for v in t[86:114]]
        tail = [int(v) for v in t[114:120]]
        # the slot: from28 limb for limb (the compiled one and the model's), unsigned limbs, the same integer
        assert w[:26] == f28 == M.unsigned(x) + M.unsigned(y), k
        assert all(0 <= v < 1 << 30 for v in w[:12] + w[13:25]) and 0 <= w[12] < 1 << 30 and 0 <= w[25] < 1 << 30
        assert M.value(w[:13]) == x and M.value(w[13:26]) == y
        # to28 of the slot: the canonical fp28 limbs again
        assert b28 == limbs28(x) + limbs28(y), k
        assert u28 == b28, k  # and without to28's carry pass (what k_fbw_accum_quad uses)
        # the flag word at word 26, zero padding behind it; both survive
        assert w[26] == flags[k] and w[27:] == [0] * 5 and tail == [flags[k]] + [0] * 5, k


def chain_points(rnd):
    """64 (m, point): both signs, an equal pair (P then P: the tangent) and an opposite pair (the sum so far, negated)"""
    pts = [(k & 1 if k % 5 else rnd.randrange(2), curve_point(rnd)) for k in range(64)]
    pts[1] = (pts[0][0], pts[0][1])                  # first point twice: equal, onto a single point
    cur = None
    for k in range(20):
        cur = affine_add(cur, neg(pts[k][1]) if pts[k][0] else pts[k][1])
    pts[20] = (0, cur)                               # equal, onto a sum
    cur = affine_add(cur, cur)
    pts[21] = (1, cur)                               # opposite: empties the chain
    pts[23] = (pts[22][0] ^ 1, pts[22][1])           # opposite, onto a single point
    return pts


def test_both_chain_add_overloads_and_both_ways_back(exe):
    rnd = random.Random(0x51071)
    beta = beta28_limbs()
    pts = chain_points(rnd)
    lines, what = ["beta " + fmt28(beta), "reset", "fin 0", "fin 1"], [None, None, ("fin", 0, None), ("fin", 1, None)]
    cur = None
    for k, (m, pt) in enumerate(pts):
        lines.append("add %d %s %s" % (m, fmt28(limbs28(mont28(pt[0]))), fmt28(limbs28(mont28(pt[1])))))
        cur = affine_add(cur, neg(pt) if m else pt)
        what.append(("add", k, cur))
        for part in (0, 1):
            lines.append("fin %d" % part)
            what.append(("fin", part, cur))
    states, signs = set(), set()
    fin_states = set()
    b = value28(beta) * R392INV % P
    assert pow(b, 3, P) == 1 and b != 1
    for w, ln in zip(what, run(exe, lines)):
        if w is None:
            continue
        t = ln.split()
        if w[0] == "add":
            st_old, st_new = int(t[0]), int(t[1])
            old, new = [int(v) for v in t[2:54]], [int(v) for v in t[54:106]]
            assert st_old == st_new and old == new, "accumulators differ after point %d" % w[1]
            assert st_new == (EMPTY if w[2] is None else st_new)
            states.add(st_new)
            signs.add(pts[w[1]][0])
        else:
            st, part, cur = int(t[0]), w[1], w[2]
            fe = [[int(v, 16) for v in t[1 + 14 * k:15 + 14 * k]] for k in range(12)]
            old, new, stored = fe[:4], fe[4:8], fe[8:]
            assert old == new, "part %d, state %d: differs from to_xyzz28 and the two fp28 products" % (part, st)
            fin_states.add((st, part))
            x, y, zzz, zz = [value28(f) * R392INV % P for f in new]
            if cur is None:
                assert st == EMPTY and all(v == 0 for f in stored for v in f)
                continue
            want = (cur[0] * b % P, P - cur[1]) if part else cur   # psi(x, y) = (beta x, -y)
            assert (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P) == want
            # what is stored: normalized, inside (0.49p, 1.51p) (g1_30s.hip.h), so inside what k_blocksum and g1::dadd take
            for f in stored:
                assert all(v < 1 << 28 for v in f[:13])
                assert Fr(49, 100) * P < value28(f) < Fr(151, 100) * P
    assert states == {EMPTY, AFFINE, XYZZ} and signs == {0, 1}
    assert fin_states == {(s, p) for s in (EMPTY, AFFINE, XYZZ) for p in (0, 1)}


def test_the_constant_for_beta_against_beta28_and_k4():
    k4, k4b = header_constant("k4"), header_constant("k4b")
    beta_mont = value28(beta28_limbs())           # beta * 2^392 mod p, canonical
    assert 0 <= beta_mont < P
    beta = beta_mont * R392INV % P
    assert pow(beta, 3, P) == 1 and beta != 1
    assert M.value(k4) % P == 4 * M.R % P
    assert M.value(k4b) % P == 4 * beta * M.R % P == M.value(k4) * beta % P == beta_mont
    # centred like k4: limbs 0..11 in [-2^29, 2^29), the value the residue nearest zero
    for c in (k4, k4b):
        assert all(-M.H <= v < M.H for v in c[:12]) and abs(M.value(c)) < P // 2 and c == M.centred(M.value(c))


def exact(l):
    """bounds of a known constant"""
    v = Fr(M.value(l), P)
    return M.B([(x, x) for x in l], v, v)


def test_the_model_admits_the_constant_and_the_negated_y():
    k4, k4b = header_constant("k4"), header_constant("k4b")
    rep = {}
    # X of a lane's sum: CHAIN_AFFINE holds unsigned limbs in [0, 1), CHAIN_XYZZ limbs in (-2^30, 2^30), (-2.2, 2.2)
    xs = [M.with_top(0, M.MASK, 0, 1), M.with_top(-M.MASK, M.MASK, -M.BOUND_X, M.BOUND_X)]
    # -Y: the negation of a centred value has limbs in [-2^29 + 1, 2^29]; (-2, 2) covers both states
    ys = [M.with_top(-M.H, M.H, -2, 2)]
    for name, ops, c in (("X * 4 beta 2^390", xs, k4b), ("X * 4 2^390", xs, k4), ("-Y * 4 2^390", ys, k4)):
        for a in ops:
            for k in (exact(c), M.b_centred(-Fr(1, 2), Fr(1, 2))):   # the constant itself, and any centred constant
                o = M.b_product([(a, k)], rep, name)
                # plus p: inside the stored-sum interval to_xyzz28 documents
                assert Fr(49, 100) < o.lo + 1 and o.hi + 1 < Fr(151, 100), name
    assert len(rep) == 3 and all(v < M.LIMIT for v in rep.values())
    # and the arithmetic itself on the limb patterns that make a column largest
    lo, hi, u = [-M.H + 1] * 12, [M.H] * 12, [M.MASK] * 12
    alt = [(-M.H + 1 if i & 1 else M.H) for i in range(12)]
    sgn = [(M.H if v >= 0 else -M.H + 1) for v in k4b[:12]]
    for a in (lo, hi, u, alt, sgn, [-v for v in sgn], [-v for v in u]):
        for top in (-(1 << 22), 1 << 22):
            for c in (k4b, k4):
                r, worst = M.mont_product("mul", [a + [top], c])
                assert worst < M.LIMIT and all(-M.H <= v < M.H for v in r[:12])
                assert (M.value(r) * M.R - M.value(a + [top]) * M.value(c)) % P == 0
