"""The prepared G2 bucket MSM (g2msm.hip) on the CPU: its four entry points named by the header, the library, the Python
module and the Rust sys crate, and the per-lane parts of the engine (g2_bucket.hip.h, host- and device-compilable) run
in a stand-alone host program:

  D  the signed base-256 recoding of every scalar of setup_model.scalar_cases() (872): sum_k d_k 256^k == s with
     |d_k| <= 128, and the entry list holds exactly the non-zero digits (none of a window whose table point is infinite);
  P  the segment plan: for bucket loads 0, 1, s - 1, s, s + 1, s^2, s^2 + 1, s^3 + 1 at segment s = 2 and 4, the
     segments of every level cover each item exactly once, and one item is left at the end;
  M  the whole path in a host model of the stages g2msm.hip enqueues (table columns and their affine form, digits, the
     count matrix and its scan, the scatter, the segment walk level by level, the weights, the tree, the sum of pass
     results, the affine output).  The g2b:: and g2:: routines are the kernels' own; the loops around them (pass
     splitting, the level loop, the count matrix) are written again in the test program, so the host code of
     g2msm.hip itself is held by the GPU tests alone.  Over 8 points of codec_model's G2 arithmetic with a point at infinity, a repeated point, a pair
     P, -P and a point of order 13 outside the subgroup, against sum_i k_i P_i on Python integers.  A mutant whose
     reduction forgets bucket 128 must be caught by the case whose scalars have the digit 128."""
import os
import random
import shutil
import subprocess

import pytest

import codec_model as CM
import setup_model as S
from test_g2_add_cpu import jac
from test_g2_lane_cpu import CSRC, P, ROOT, R392, fe, value

R = S.R
NAMES = (("kzgamd_g2_msm_new", 4), ("kzgamd_g2_msm_free", 1), ("kzgamd_g2_msm", 5), ("kzgamd_g2_msm_info", 6))

PROGRAM = r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "g2_28.hip.h"
#include "g2_bucket.hip.h"
using ff::u32;
using fp28::Fe;
using g2::F2;
static bool rd(Fe& r) { for (int i = 0; i < 14; ++i) if (scanf("%x", &r.v[i]) != 1) return false; return true; }
static bool rd2(F2& r) { return rd(r.c0) && rd(r.c1); }
static bool rdj(g2::Jac& p) { return rd2(p.x) && rd2(p.y) && rd2(p.z); }
static bool rdk(ff::Fr& k) { for (int w = 0; w < 8; ++w) if (scanf("%x", &k.v[w]) != 1) return false; return true; }
static void raw(const Fe& a) { for (int i = 0; i < 14; ++i) printf("%x ", a.v[i]); }
static void scan(std::vector<u32>& v) { u32 run = 0; for (u32& x : v) { const u32 c = x; x = run; run += c; } }

// g2msm.hip on the host, stage by stage: every kernel is a loop over its lanes
struct Msm {
    size_t np = 0;
    std::vector<g2::AffPt> tab;
    std::vector<u32> inf_mask;
    void build(const std::vector<g2::Jac>& pts) {  // k_g2msm_columns, k_g2msm_affine
        np = pts.size();
        tab.resize(32 * np);
        inf_mask.assign(np, 0);
        for (size_t i = 0; i < np; ++i) {
            g2::Jac p = pts[i];
            for (int k = 0; k < g2b::NWIN; ++k) {
                g2::AffPt a;
                g2::to_affine(a, p);
                tab[k * np + i] = a;
                if (a.flags & 1) inf_mask[i] |= 1u << k;
                if (k + 1 < g2b::NWIN) g2b::next_window(p);
            }
        }
    }
    void pass(std::vector<g2::Jac>& acc, const std::vector<ff::Fr>& sc, size_t n, size_t b0, size_t nb, size_t i0, size_t i1, u32 seg,
              bool mutant) const {
        const size_t npts = i1 - i0, nblk = (npts + 63) / 64, K = nb * 128, m = K * nblk + 1;
        std::vector<u32> cnt(m, 0);
        for (size_t by = 0; by < nb; ++by)  // k_g2msm_count
            for (size_t i = i0; i < i1; ++i)
                g2b::for_each_entry(sc[(b0 + by) * n + i], (u32)i, (u32)np, inf_mask[i],
                                    [&](u32 bucket, u32) { ++cnt[(by * 128 + bucket - 1) * nblk + (i - i0) / 64]; });
        scan(cnt);
        std::vector<u32> entries(cnt[m - 1]), at(cnt);
        for (size_t by = 0; by < nb; ++by)  // k_g2msm_scatter
            for (size_t i = i0; i < i1; ++i)
                g2b::for_each_entry(sc[(b0 + by) * n + i], (u32)i, (u32)np, inf_mask[i],
                                    [&](u32 bucket, u32 v) { entries[at[(by * 128 + bucket - 1) * nblk + (i - i0) / 64]++] = v; });
        std::vector<u32> in_off(K + 1), out_off(K + 1);
        for (size_t key = 0; key <= K; ++key) in_off[key] = cnt[key * nblk];  // k_g2msm_key_offsets
        std::vector<g2::Jac> in, out;
        size_t most = npts * 32;
        for (int level = 0;; ++level) {
            for (size_t key = 0; key < K; ++key) out_off[key] = g2b::segments(in_off[key + 1] - in_off[key], seg);
            out_off[K] = 0;
            scan(out_off);
            out.assign(out_off[K], g2::Jac());
            for (u32 s = 0; s < out_off[K]; ++s) {  // k_g2msm_accum, k_g2msm_level
                const u32 key = g2b::key_of(out_off.data(), (u32)K, s);
                u32 lo, hi;
                g2b::segment_range(in_off[key + 1] - in_off[key], seg, s - out_off[key], lo, hi);
                if (level == 0) g2b::chain_entries(out[s], tab.data(), entries.data() + in_off[key] + lo, hi - lo);
                else g2b::chain_partials(out[s], in.data() + in_off[key] + lo, hi - lo);
            }
            most = (most + seg - 1) / seg;
            if (most <= 1) break;
            in.swap(out);
            in_off = out_off;
        }
        std::vector<g2::Jac> w(K);
        for (size_t key = 0; key < K; ++key) {  // k_g2msm_weigh
            if (out_off[key + 1] != out_off[key] && !(mutant && key % 128 == 127)) g2b::weigh(w[key], out[out_off[key]], (u32)(key % 128) + 1);
            else g2::set_inf(w[key]);
        }
        for (size_t by = 0; by < nb; ++by) {  // k_g2msm_reduce
            g2::Jac slots[64];
            for (int t = 0; t < 64; ++t) slots[t] = w[by * 128 + t];
            for (int half = 64; half >= 1; half >>= 1)
                for (int t = 0; t < half; ++t) {
                    g2::Jac a = slots[t];
                    g2::add(a, half == 64 ? w[by * 128 + t + 64] : slots[t + half]);
                    slots[t] = a;
                }
            g2::Jac r = slots[0];
            g2::add(r, acc[b0 + by]);
            acc[b0 + by] = r;
        }
    }
    void run(const std::vector<ff::Fr>& sc, size_t n, size_t nbatch, u32 seg, size_t pass_entries, bool mutant) const {  // kzgamd_g2_msm
        std::vector<g2::Jac> acc(nbatch);
        for (auto& a : acc) g2::set_inf(a);
        const size_t per_item = n * 32;
        if (n == 0) {
        } else if (per_item <= pass_entries) {
            const size_t per = pass_entries / per_item;
            for (size_t b0 = 0; b0 < nbatch; b0 += per) pass(acc, sc, n, b0, nbatch - b0 < per ? nbatch - b0 : per, 0, n, seg, mutant);
        } else {
            const size_t pts = pass_entries / 32;
            for (size_t b = 0; b < nbatch; ++b)
                for (size_t i0 = 0; i0 < n; i0 += pts) pass(acc, sc, n, b, 1, i0, n - i0 < pts ? n : i0 + pts, seg, mutant);
        }
        for (size_t b = 0; b < nbatch; ++b) {  // k_g2msm_out
            g2::AffPt a;
            g2::to_affine(a, acc[b]);
            printf("%d ", (int)(a.flags & 1));
            raw(a.x.c0); raw(a.x.c1); raw(a.y.c0); raw(a.y.c1);
        }
        printf("\n");
    }
};

int main() {
    char op[16];
    Msm msm;
    while (scanf("%15s", op) == 1) {
        if (op[0] == 'D') {  // D k i npoints inf_mask: the 32 signed digits, then the entries
            ff::Fr k;
            u32 i, np, mask, carry = 0;
            if (!rdk(k) || scanf("%u %u %x", &i, &np, &mask) != 3) return 2;
            for (int w = 0; w < g2b::NWIN; ++w) {
                u32 neg;
                const u32 d = g2b::signed_digit(k, w, carry, neg);
                if (neg != 0 && neg != 0xffffffffu) return 3;
                printf("%d ", neg ? -(int)d : (int)d);
            }
            printf("%u ", carry);
            g2b::for_each_entry(k, i, np, mask, [](u32 bucket, u32 v) { printf("%u %u ", bucket, v); });
            printf("\n");
        } else if (op[0] == 'P') {  // P c seg: per level "c lo hi lo hi ... |"
            u32 c, seg;
            if (scanf("%u %u", &c, &seg) != 2) return 2;
            u32 most = c;
            for (;;) {
                printf("%u ", c);
                const u32 ns = g2b::segments(c, seg);
                for (u32 j = 0; j < ns; ++j) {
                    u32 lo, hi;
                    g2b::segment_range(c, seg, j, lo, hi);
                    printf("%u %u ", lo, hi);
                }
                printf("| ");
                c = ns;
                most = (most + seg - 1) / seg;
                if (most <= 1) break;
            }
            printf("%u\n", c);
        } else if (op[0] == 'T') {  // T np, the points: the table
            int np;
            if (scanf("%d", &np) != 1) return 2;
            std::vector<g2::Jac> pts(np);
            for (auto& p : pts) if (!rdj(p)) return 2;
            msm.build(pts);
            for (u32 m : msm.inf_mask) printf("%x ", m);
            printf("\n");
        } else if (op[0] == 'M') {  // M n nbatch seg pass_entries mutant, the scalars (plain)
            size_t n, nbatch, pass;
            u32 seg;
            int mutant;
            if (scanf("%zu %zu %u %zu %d", &n, &nbatch, &seg, &pass, &mutant) != 5 || n > msm.np) return 2;
            std::vector<ff::Fr> sc(n * nbatch);
            for (auto& k : sc) if (!rdk(k)) return 2;
            msm.run(sc, n, nbatch, seg, pass, mutant != 0);
        } else return 4;
    }
    return 0;
}
'''


def words(k):
    return " ".join("%x" % ((k >> (32 * w)) & 0xffffffff) for w in range(8))


def compile_program(tmp_path, name, extra=(), cxx=None):
    cxx = cxx or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / (name + ".cpp")
    src.write_text(PROGRAM)
    exe = tmp_path / name
    built = subprocess.run([cxx, "-O2", "-std=c++17"] + list(extra) + ["-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    return exe


def run_program(exe, lines):
    run = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0 and "runtime error" not in run.stderr, (run.returncode, run.stderr[-2000:])
    out = run.stdout.strip().split("\n")
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return compile_program(tmp_path_factory.mktemp("g2msm"), "g2msm_host")


def test_header_library_python_module_and_rust_sys_crate_name_the_entry_points():
    from conftest import load_package
    from test_host_cpu import _c_prototypes, _rust_externs

    protos = _c_prototypes()
    ext = _rust_externs(os.path.join(ROOT, "rust-kzg_amd", "rust", "src", "lib.rs"))
    pkg = load_package("product")
    L = pkg.lib()
    for name, nargs in NAMES:
        assert len(protos[name]) == nargs, (name, protos[name])
        assert len(ext[name]) == nargs, (name, ext[name])
        assert name in pkg.EXPORTS and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert callable(pkg.G2Msm) and callable(pkg.G2Msm.g2_msm) and callable(pkg.G2Msm.close)
    keys = pkg.tuning_keys()
    assert "g2msm_segment" not in keys and "g2msm_pass_entries" not in keys
    import importlib.util
    spec = importlib.util.spec_from_file_location("rust_kzg_amd_build_g2msm", os.path.join(ROOT, "rust-kzg_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "g2msm.hip" in b.SOURCES and "g2_bucket.hip.h" in b.HEADERS


def check_recoding(exe, cases, point, npoints, mask):
    out = run_program(exe, ["D %s %d %d %x" % (words(k), point, npoints, mask) for k in cases])
    for k, ln in zip(cases, out):
        t = [int(x) for x in ln.split()]
        digits, carry, rest = t[:32], t[32], t[33:]
        assert carry == 0, hex(k)
        assert all(abs(d) <= 128 for d in digits), hex(k)
        assert sum(d << (8 * w) for w, d in enumerate(digits)) == k, hex(k)
        want = [(abs(d), (w * npoints + point) | (0x80000000 if d < 0 else 0)) for w, d in enumerate(digits) if d and not (mask >> w) & 1]
        assert list(zip(rest[0::2], rest[1::2])) == want, hex(k)
    return out


def test_recoding_identity_and_the_entries_of_every_scalar_case(exe):
    cases = S.scalar_cases()
    assert len(cases) == 872
    check_recoding(exe, cases, 5, 9, 0)
    check_recoding(exe, cases, 0, 1, 0)
    check_recoding(exe, cases[:200], (1 << 20) - 1, 1 << 20, 0)  # the largest index of a table of 2^20 points: 2^25 - 1
    # windows whose table point is infinite yield no entry
    check_recoding(exe, cases, 2, 7, 0xffffffff)
    check_recoding(exe, cases, 2, 7, 0x80000001)
    check_recoding(exe, cases, 2, 7, 0x00010100)


@pytest.mark.parametrize("seg", [2, 4])
def test_segments_of_every_level_cover_each_item_once(exe, seg):
    loads = [0, 1, seg - 1, seg, seg + 1, seg * seg, seg * seg + 1, seg ** 3 + 1]
    out = run_program(exe, ["P %d %d" % (c, seg) for c in loads])
    for c, ln in zip(loads, out):
        *levels, last = ln.split("|")
        assert int(last) == (1 if c else 0), (c, ln)
        want_c, nlevels = c, 0
        for lv in levels:
            t = [int(x) for x in lv.split()]
            assert t[0] == want_c, (c, ln)
            ranges = list(zip(t[1::2], t[2::2]))
            assert len(ranges) == -(-want_c // seg)
            covered = [i for lo, hi in ranges for i in range(lo, hi)]
            assert covered == list(range(want_c)), (c, ln)  # every item once, in order
            assert all(0 < hi - lo <= seg for lo, hi in ranges), (c, ln)
            want_c = len(ranges)
            nlevels += 1
        # as many levels as the largest load needs, and no more than one beyond
        need = 1
        while seg ** need < c:
            need += 1
        assert nlevels == need, (c, ln)


# ---- the whole path
def points_and_affine():
    rnd = random.Random(0x62)
    rz = lambda: (rnd.randrange(P), rnd.randrange(P))
    g = CM.G2
    q = CM.mul(0x1234567, g)
    t = CM.torsion_point(13)
    aff = [g, CM.mul(7, g), None, CM.mul(7, g), q, CM.neg(q), t, CM.mul(12, g)]
    zs = [(1, 0), rz(), None, rz(), rz(), rz(), rz(), rz()]
    return aff, [jac(a, z, [0] * 6) for a, z in zip(aff, zs)]


_mul_cache = {}


def kp(i, k, aff):
    if (i, k) not in _mul_cache:
        _mul_cache[(i, k)] = CM.mul(k, aff[i]) if aff[i] is not None and k else None
    return _mul_cache[(i, k)]


def expected(aff, scalars, n, nbatch):
    out = []
    for b in range(nbatch):
        acc = None
        for i in range(n):
            acc = CM.add(acc, kp(i, scalars[b * n + i], aff))
        out.append(acc)
    return out


def parse_outputs(ln, nbatch):
    t = [int(x, 16) for x in ln.split()]
    assert len(t) == nbatch * 57
    rinv = pow(R392, -1, P)
    out = []
    for b in range(nbatch):
        rec = t[57 * b:57 * b + 57]
        comps = [rec[1 + 14 * c:15 + 14 * c] for c in range(4)]
        if rec[0]:
            assert all(x == 0 for c in comps for x in c)
            out.append(None)
        else:
            assert all(value(c) < P for c in comps), "canonical"
            v = [value(c) * rinv % P for c in comps]
            out.append(((v[0], v[1]), (v[2], v[3])))
    return out


def msm_cases():
    rnd = random.Random(0x9b)
    rs = lambda n: [rnd.randrange(R) for _ in range(n)]
    d128 = [128, 128 << 8, 129, 255, 256, R - 1, (128 << 16) | 128, 0x80 << 248 >> 8]
    cases = []  # (tag, n, nbatch, scalars)
    cases.append(("random", 8, 1, rs(8)))
    cases.append(("the digit 128", 8, 1, d128))
    cases.append(("all one: 7 entries in one bucket, P - P and a repeated point", 8, 1, [1] * 8))
    cases.append(("32 bytes of 1: every entry in bucket 1", 8, 1, [int.from_bytes(b"\x01" * 32, "little")] * 8))
    cases.append(("all zero", 8, 1, [0] * 8))
    cases.append(("P and -P under equal scalars", 6, 1, [0, 0, 5, 0] + [rnd.randrange(R)] * 2))
    cases.append(("order 13 alone", 7, 1, [0] * 6 + [13 * 256 ** 7]))
    cases.append(("a prefix", 3, 1, rs(3)))
    cases.append(("one point", 1, 1, rs(1)))
    cases.append(("no point", 0, 2, []))
    cases.append(("a batch: random, zero, one", 8, 3, rs(8) + [0] * 8 + [1] * 8))
    return cases


def test_the_whole_path_on_the_host_against_python_integers(exe):
    aff, pts = points_and_affine()
    lines = ["T %d\n%s" % (len(pts), "\n".join(" ".join(fe(c) for c in p) for p in pts))]
    checks = []
    for tag, n, nbatch, sc in msm_cases():
        for seg, pass_entries in ((2, 1 << 25), (4, 1 << 25), (16, 1 << 25), (4, 32), (2, 64), (16, 96)):
            lines.append("M %d %d %d %d 0 %s" % (n, nbatch, seg, pass_entries, " ".join(words(k) for k in sc)))
            checks.append((tag, n, nbatch, sc, seg, pass_entries))
    # the mutant: bucket 128 forgotten
    mut = msm_cases()[1]
    lines.append("M %d %d 4 %d 1 %s" % (mut[1], mut[2], 1 << 25, " ".join(words(k) for k in mut[3])))
    out = run_program(exe, lines)
    # only the point at infinity has infinite table entries: E'(Fp2) has odd order, so no doubling ends at infinity
    assert [int(x, 16) for x in out[0].split()] == [0, 0, 0xffffffff, 0, 0, 0, 0, 0]
    seen_inf = False
    for (tag, n, nbatch, sc, seg, pass_entries), ln in zip(checks, out[1:]):
        want = expected(aff, sc, n, nbatch)
        assert parse_outputs(ln, nbatch) == want, (tag, seg, pass_entries)
        seen_inf = seen_inf or None in want
        if tag in ("all zero", "P and -P under equal scalars", "order 13 alone", "no point"):
            assert all(w is None for w in want), tag
    assert seen_inf
    want = expected(aff, mut[3], mut[1], mut[2])
    assert any(abs(d) == 128 for k in mut[3] for d in _digits(k))
    assert parse_outputs(out[-1], mut[2]) != want, "a reduction without bucket 128 passed the case with the digit 128"


def _digits(k):
    carry, out = 0, []
    for w in range(32):
        d = ((k >> (8 * w)) & 0xff) + carry
        carry = 1 if d > 128 else 0
        out.append(d - 256 if carry else d)
    return out


def test_no_undefined_behaviour_in_the_host_build(tmp_path):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("g++")
    flags = ["-g", "-fsanitize=signed-integer-overflow,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([cxx, "-O1", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + (probed.stderr.strip().split("\n") or [""])[-1])
    san = compile_program(tmp_path, "g2msm_ubsan", flags, cxx)
    aff, pts = points_and_affine()
    lines = ["T %d\n%s" % (len(pts), "\n".join(" ".join(fe(c) for c in p) for p in pts))]
    lines += ["D %s 3 8 0" % words(k) for k in S.scalar_cases()[:64]] + ["P 65 4"]
    for tag, n, nbatch, sc in msm_cases():
        lines.append("M %d %d 4 64 0 %s" % (n, nbatch, " ".join(words(k) for k in sc)))
    run_program(san, lines)


@pytest.mark.parametrize("exact", [False, True])
def test_g2msm_cross_compiles_for_gfx950_with_the_products_flags(tmp_path, exact):
    import importlib.util
    spec = importlib.util.spec_from_file_location("rust_kzg_amd_build_g2msm_x", os.path.join(ROOT, "rust-kzg_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    out = str(tmp_path / "g2msm.o")
    p = subprocess.run([b.hipcc_path()] + b.COMPILE_FLAGS + (["-DKZGAMD_FORCE_EXACT_TESTS"] if exact else []) +
                       ["-fPIC", "-c", os.path.join(CSRC, "g2msm.hip"), "-o", out], capture_output=True, text=True)
    assert p.returncode == 0 and os.path.getsize(out) > 0, p.stderr[-3000:]
