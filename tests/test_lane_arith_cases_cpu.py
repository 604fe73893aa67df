"""The CPU side of the lane-arithmetic contract tests (tests/test_lane_arith_gpu.py runs the cases on the device):
the case lists build with every generator's preconditions holding, the model's curve arithmetic is the oracle's, the
device harness cross-compiles for gfx950 under each of its define sets, and the single-lane routines of g1_28.hip.h —
which compile for the host — pass their share of the cases here, at the bounds of points the wide code stored."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import lane_harness as H
import lane_model as M


@pytest.fixture(scope="module")
def blocks():
    return M.all_cases()


def test_case_lists_build_and_their_preconditions_hold(blocks):
    """all_cases() runs every generator, and every generator asserts the contract of the routine it feeds"""
    total = sum(len(v) for v in blocks.values())
    print("lane arithmetic cases per op:", ", ".join("%s %d" % (op, len(v)) for op, v in blocks.items()), "- total", total)
    assert set(blocks) == set(M.OPS)
    assert 2000 < total < 12000
    # the edges the issue names are there
    def rows(op):
        return [c.words[i:i + 14] for c in blocks[op] for i in range(0, len(c.words), 14)]

    assert [M.FULL] + [M.M28] * 12 + [0x1a011] in rows("wnorm"), "the longest ripple"
    assert [(1 << 31) - 1] * 14 in rows("wnorm_full") and [M.FULL] * 13 + [0] in rows("wnorm_full")
    zero_multiples = sum(1 for c in blocks["is_zero"] if M.value(c.words[:14]) % M.P == 0)
    assert zero_multiples >= 64
    tags = {c.tag for c in blocks["dadd"]}
    assert {"P+Q", "inf+Q", "P+inf", "inf+inf", "P+P same z", "P+P other z", "P+(-P) same z", "P+(-P) other z"} <= tags
    # the text form round-trips through the decoder's expectations
    text = M.encode(blocks)
    assert text.count("\n") == total + len(blocks)


def test_checkers_reject_a_spoilt_result():
    """a checker that accepts anything is no checker: the expected result of a point case passes, one limb off fails"""
    rnd = random.Random(7)
    p, q = M.sample_points()[1], M.sample_points()[9]
    want = M.aff_add(p, q)
    limbs = M.wide_reps(want, rnd, "top")
    out = []
    for l in limbs:
        out += (l + [0, 0]) * 4
    M.check_wide_point(out, want)
    for spoil in (37, 64 + 3, 128 + 16 + 14, 192 + 48):  # a limb of one row, a limb of y, lane 14 of a row, zz
        bad = list(out)
        bad[spoil] += 1
        with pytest.raises(AssertionError):
            M.check_wide_point(bad, want)
    with pytest.raises(AssertionError):
        M.check_wide_point(out, p)
    with pytest.raises(AssertionError):
        M.check_wide_point(out, None)


def test_model_curve_arithmetic_is_the_oracles(oracle):
    """the dozen lines of affine arithmetic in lane_model.py against the oracle's G1 on a handful of points"""
    import oracle_ffi as O

    L = oracle.lib()
    g = O.G1()
    L.og1_generator(C.byref(g))

    def comp(p):
        buf = C.create_string_buffer(48)
        L.og1_compress(buf, C.byref(p))
        return buf.raw.hex()

    def omul(p, k):
        r, kf = O.G1(), O.fr_from_int(k % O.R)
        L.og1_mul(C.byref(r), C.byref(p), C.byref(kf))
        return r

    gen = M.generator()
    assert M.compress(gen) == comp(g)
    rnd = random.Random(99)
    for k, j in [(1, 1), (2, 3), (5, 5), (rnd.randrange(O.R), rnd.randrange(O.R)), (rnd.randrange(O.R), 1), (7, O.R - 7)]:
        a, b = M.aff_mul(k, gen), M.aff_mul(j, gen)
        oa, ob = omul(g, k), omul(g, j)
        assert M.compress(a) == comp(oa) and M.compress(b) == comp(ob)
        s = O.G1()
        L.og1_add_or_dbl(C.byref(s), C.byref(oa), C.byref(ob))
        assert M.compress(M.aff_add(a, b)) == comp(s), (k, j)
        assert M.compress(M.aff_dbl(a)) == comp(omul(g, 2 * k))
        assert M.compress(M.aff_add(a, M.aff_neg(a))) == comp(O.G1())
        assert M.decompress(M.compress(a)) == a
    # lifting to XYZZ and back is the identity on the point, whatever z and the representatives
    for pt in M.sample_points()[:4]:
        for which in ("low", "top", "mixed"):
            limbs = M.wide_reps(pt, rnd, which)
            assert M.affine_of(*[M.value(l) for l in limbs]) == pt


@pytest.fixture(scope="module")
def cross_compiled(tmp_path_factory):
    if not os.path.exists(H.product_build().hipcc_path()):
        pytest.skip("no hipcc on this machine")
    sets = dict(H.DEFINE_SETS)
    sets.update(H.PLANTED)
    return H.compile_all(tmp_path_factory.mktemp("lane_check"), sets)


@pytest.mark.parametrize("name", list(H.DEFINE_SETS) + list(H.PLANTED))
def test_device_harness_cross_compiles_for_gfx950(cross_compiled, name):
    """a header change that breaks tests/device_checks/lane_check.hip shows here, on a machine without a GPU"""
    built, errors = cross_compiled
    assert name in built, errors.get(name)
    cmd = H.compile_command("x", H.DEFINE_SETS.get(name, H.PLANTED.get(name)))
    assert "--offload-arch=gfx950" in cmd and "-O3" in cmd and "-std=c++17" in cmd


HOST_CHECKER = r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "g1_28.hip.h"
using g1::Xyzz;
using ff::u32;
static Xyzz pt(const u32* w) { Xyzz p; memcpy(&p, w, sizeof p); return p; }
static fp28::Fe fe(const u32* w) { fp28::Fe a; memcpy(&a, w, sizeof a); return a; }
int main() {
    static_assert(sizeof(Xyzz) == 56 * 4, "layout");
    char op[64];
    unsigned long n;
    while (scanf("%63s %lu", op, &n) == 2) {
        int nin = !strcmp(op, "one_dadd") || !strcmp(op, "one_dadd_unequal") ? 112 : !strcmp(op, "one_dbl_k") ? 57
                  : !strcmp(op, "one_madd") ? 84 : !strcmp(op, "one_chain_add") ? 86 : 56;
        printf("%s %lu\n", op, n);
        for (unsigned long k = 0; k < n; ++k) {
            std::vector<u32> in(nin), out(57, 0xA5A5A5A5u);
            for (u32& w : in) if (scanf("%x", &w) != 1) { printf("input\n"); return 1; }
            Xyzz acc = pt(in.data());
            u32 flag = 0;
            bool point = true;
            if (!strcmp(op, "one_dadd")) g1::dadd(acc, pt(in.data() + 56));
            else if (!strcmp(op, "one_dadd_unequal")) flag = g1::dadd_unequal(acc, pt(in.data() + 56)) ? 1 : 0;
            else if (!strcmp(op, "one_dbl_k")) g1::dbl_k(acc, (int)in[56]);
            else if (!strcmp(op, "one_madd")) g1::madd(acc, fe(in.data() + 56), fe(in.data() + 70));
            else if (!strcmp(op, "one_chain_add")) { flag = in[56]; g1::chain_add(acc, flag, fe(in.data() + 57), fe(in.data() + 71), in[85]); }
            else if (!strcmp(op, "one_reduce_xy")) g1::reduce_xy(acc);
            else if (!strcmp(op, "grp_dbl1")) g1::dbl(acc);
            else if (!strcmp(op, "one_to_blst")) {
                ff::Fp j[3];
                g1::to_blst_jacobian(j, acc);
                for (int c = 0; c < 3; ++c) for (int i = 0; i < 12; ++i) out[1 + 12 * c + i] = j[c].v[i];
                point = false;
            } else { printf("unknown op\n"); return 1; }
            out[0] = flag;
            if (point) memcpy(out.data() + 1, &acc, sizeof acc);
            for (u32 w : out) printf("%x ", w);
            printf("\n");
        }
    }
    printf("done\n");
    return 0;
}
'''
HOST_OPS = ("one_dadd", "one_dadd_unequal", "one_dbl_k", "one_madd", "one_chain_add", "one_to_blst", "one_reduce_xy", "grp_dbl1")


@pytest.mark.parametrize("exact", [False, True])
def test_single_lane_consumers_of_wide_stored_points_on_the_host(tmp_path, blocks, exact):
    """g1_28.hip.h compiled for the host on the cases the device harness runs for it: g1::dadd, dadd_unequal, dbl_k,
    to_blst_jacobian and reduce_xy on points with X, Y just under 18p (what g1w::store may write), madd, chain_add and
    dbl at their own bounds; with and without the filter of the exact zero test."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    src = tmp_path / "one_lane_check.cpp"
    src.write_text(HOST_CHECKER)
    exe = tmp_path / "one_lane_check"
    subprocess.check_call([cxx, "-O1", "-std=c++17"] + (["-DKZGAMD_FORCE_EXACT_TESTS"] if exact else []) + ["-I", H.CSRC, str(src), "-o", str(exe)])
    mine = {op: blocks[op] for op in HOST_OPS}
    out = subprocess.run([str(exe)], input=M.encode(mine), capture_output=True, text=True, check=True, timeout=120).stdout
    outs = M.decode(out, mine)
    bad = M.failures(mine, outs)
    assert not bad, "%d of %d cases fail, the first: %s" % (len(bad), sum(len(v) for v in mine.values()), bad[:5])
