"""What the compiler makes of fp30s.hip.h / g1_30s.hip.h for gfx950: a host-only check (cross-compilation to assembly, no
GPU) of the static instruction counts the speed of k_fbw_accum rests on.  Correctness does not depend on any of them;
a toolchain that stops cooperating would lose the gain silently, so it fails here instead.

A stand-alone kernel with the loop of k_fbw_accum (one inlined g1s::chain_add, then g1s::to_xyzz28) holds 32
Montgomery reductions: 9 in the addition onto a sum, 5 in the one onto a single point, 7 in each of the two sites of the
tangent, 4 on the way back.  Per reduction 13 lower and 12 upper columns.
  v_mad_i64_i32   every product of two limbs and of a digit and a limb of p is ONE signed multiply-add:
                  3 055 + 1 703 + 2 * 1 963 + 1 352 = 10 036, and 52 in the four exact zero tests;
  v_mul_lo_u32    one per quotient digit (32 * 13 = 416 at most; a few fold away).  A signed product whose operand was
                  widened in another block costs two more each — hundreds (g1_30s.hip.h, chain_add);
  v_lshl_add_u64  one 64-bit addition per column but the first (32 * 24): the seeds of fp30s::seeds() ride in the first
                  multiply-add of every column.  As literals they cost a second addition per column;
  registers       at most 256 and no scratch, as the kernel's two waves per SIMD need."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-kzg_amd"))

KERNEL = r'''
#include "g1_30s.hip.h"
extern "C" __global__ void __launch_bounds__(256) kchain(const g1::WidePt* tab, g1::Xyzz* out, const unsigned* sel, int n) {
    const fp30s::Seeds sd = fp30s::seeds();
    g1s::Xyzz acc;
    g1s::set_inf(acc);
    ff::u32 st = g1::CHAIN_EMPTY;
    for (int i = 0; i < n; ++i) {
        const unsigned e = sel[threadIdx.x * n + i];
        const g1::WidePt pk = tab[e & 0x7fffffffu];
        if (pk.pad[0]) continue;
        g1s::chain_add(acc, st, pk.x, pk.y, 0u - (e >> 31), sd);
    }
    g1::Xyzz sum;
    g1s::to_xyzz28(sum, acc, st, sd);
    out[threadIdx.x] = sum;
}
'''


def test_static_counts_of_the_addition_chain(tmp_path):
    import build as B
    hipcc = B.hipcc_path()
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: " + hipcc)
    src = tmp_path / "kchain.hip"
    src.write_text(KERNEL)
    asm = tmp_path / "kchain.s"
    subprocess.check_call([hipcc] + B.COMPILE_FLAGS + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"),
                           str(src), "-o", str(asm)], stderr=subprocess.DEVNULL)
    text = asm.read_text()
    ops = {}
    for m in re.finditer(r"^\s+([vs]_\w+|scratch_\w+)", text, re.M):
        ops[m.group(1)] = ops.get(m.group(1), 0) + 1
    print({k: ops.get(k, 0) for k in ("v_mad_i64_i32", "v_mad_u64_u32", "v_mul_lo_u32", "v_lshl_add_u64", "v_ashrrev_i64")})
    assert ops.get("v_mad_i64_i32", 0) == 10036 + 52
    assert ops.get("v_mad_u64_u32", 0) <= 40          # addressing only
    assert ops.get("v_mul_lo_u32", 0) <= 32 * 13 + 8
    assert ops.get("v_ashrrev_i64", 0) == 32 * 24
    assert ops.get("v_lshl_add_u64", 0) <= 32 * 24 + 8
    assert not any(k.startswith("scratch_") for k in ops)
    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", text).group(1)) == 0
    agpr = re.search(r"\.agpr_count:\s*(\d+)", text)
    assert int(re.search(r"\.vgpr_count:\s*(\d+)", text).group(1)) + (int(agpr.group(1)) if agpr else 0) <= 256
