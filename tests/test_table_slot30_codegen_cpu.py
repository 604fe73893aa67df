"""What the compiler makes of the wide table's slot in the chain's own limbs (g1s::WidePt30) for gfx950: a host-only check
(cross-compilation to assembly, no GPU), in the shape of test_fp30s_codegen_cpu.py, of what the change is for.
Correctness does not depend on any of it.

The stand-alone loop of k_fbw_accum<.., true> (one inlined g1s::chain_add, then the way back and psi on the odd lanes)
in three forms:
  old    the former slot (g1::WidePt) through the overload over fp28::Fe, which re-slices x and y at every addition;
         g1s::to_xyzz28 and then the two fp28 products of psi (x * beta28(), neg<8>(y) * one()) — what the kernel was;
  new    g1s::WidePt30 through the overload over fp30s::Fe; g1s::to_xyzz28 with the lane's part — what the kernel is;
  mixed  the former slot and overload with the new way back: it differs from `old` only behind the loop and from `new`
         only inside it, which is how the two savings are told apart.
Asserted:
  v_mad_i64_i32   new == old: no product of the chain or of the way back was added or lost;
  v_mad_u64_u32   the two fp28 products are unsigned multiply-adds: old - mixed of them (at most 2 * 2 * 14^2), and new
                  has exactly that many fewer than old — what is left is addressing;
  VALU            new has at least 60 fewer than mixed: the re-slicing was 2 * 13 * 3 = 78 instructions at the one site
                  chain_add is inlined at (profiles/NOTES.md, section 34); sixty leaves room for scheduling;
  gathers         one 16-byte global load fewer at the one gather: words 0..26 of a slot instead of 0..28;
  registers       at most 256 and no scratch, as the kernel's two waves per SIMD need.

The stand-alone loop does not show what the kernel's own loops do to the register allocation (without g1s::hold the
stand-alone loop takes 222 registers and k_fbw_accum 302), so a second test compiles k_fbw_accum itself, cut out of
msm.hip with the few declarations it needs, in the headline instantiation and in one without the GLV split, and holds
both to 256 registers and no scratch."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rust-kzg_amd"))

KERNEL = r'''
#include "g1_30s.hip.h"
#define FORM_%(form)s 1
__device__ __forceinline__ fp28::Fe beta28() {  // as in msm.hip
    constexpr ff::u32 t[14] = {0xa75929au, 0x681b798u, 0x22a3e9du, 0xabc02bfu, 0x4e5bb45u, 0x55e6e7eu, 0x4814117u,
                               0x6d04f1bu, 0xae3387du, 0x54acb0cu, 0xa4c74bu, 0x56138b5u, 0xb64e066u, 0x76f2u};
    fp28::Fe b;
#pragma unroll
    for (int k = 0; k < 14; ++k) b.v[k] = t[k];
    return b;
}
#if defined(FORM_new)
typedef g1s::WidePt30 Slot;
__device__ __forceinline__ bool at_infinity(const Slot& s) { return s.flags != 0; }
#else
typedef g1::WidePt Slot;
__device__ __forceinline__ bool at_infinity(const Slot& s) { return s.pad[0] != 0; }
#endif
extern "C" __global__ void __launch_bounds__(256) kchain(const Slot* tab, g1::Xyzz* out, const unsigned* sel, int n) {
    const fp30s::Seeds sd = fp30s::seeds();
    const ff::u32 part = threadIdx.x & 1;
    g1s::Xyzz acc;
    g1s::set_inf(acc);
    ff::u32 st = g1::CHAIN_EMPTY;
    for (int i = 0; i < n; ++i) {
        const unsigned e = sel[threadIdx.x * n + i];
        Slot pk = tab[e & 0x7fffffffu];
        if (at_infinity(pk)) continue;
#if defined(FORM_new)
        g1s::hold(pk);  // as the kernel does (g1_30s.hip.h says why)
#endif
        g1s::chain_add(acc, st, pk.x, pk.y, 0u - (e >> 31), sd);
    }
    g1::Xyzz sum;
#if defined(FORM_old)
    g1s::to_xyzz28(sum, acc, st, sd);
    if (part && st != g1::CHAIN_EMPTY) {
        sum.x = fp28::mul(sum.x, beta28());
        sum.y = fp28::mul(fp28::neg<8>(sum.y), fp28::one());
    }
#else
    g1s::to_xyzz28(sum, acc, st, part, sd);
#endif
    out[threadIdx.x] = sum;
}
'''


def compile_form(B, tmp_path, form):
    src = tmp_path / ("kchain_%s.hip" % form)
    src.write_text(KERNEL % {"form": form})
    asm = tmp_path / ("kchain_%s.s" % form)
    subprocess.check_call([B.hipcc_path()] + B.COMPILE_FLAGS + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"),
                           str(src), "-o", str(asm)], stderr=subprocess.DEVNULL)
    text = asm.read_text()
    ops = {}
    for m in re.finditer(r"^\s+([vs]_\w+|scratch_\w+|global_\w+)", text, re.M):
        ops[m.group(1)] = ops.get(m.group(1), 0) + 1
    agpr = re.search(r"\.agpr_count:\s*(\d+)", text)
    return {"ops": ops,
            "valu": sum(v for k, v in ops.items() if k.startswith("v_")),
            "scratch": int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", text).group(1)),
            "regs": int(re.search(r"\.vgpr_count:\s*(\d+)", text).group(1)) + (int(agpr.group(1)) if agpr else 0)}


def test_static_counts_old_slot_against_new_slot(tmp_path):
    import build as B
    if not os.path.exists(B.hipcc_path()):
        pytest.skip("no hipcc: " + B.hipcc_path())
    forms = ("old", "new", "mixed")
    with ThreadPoolExecutor(3) as pool:
        old, new, mixed = pool.map(lambda f: compile_form(B, tmp_path, f), forms)
    for f, r in zip(forms, (old, new, mixed)):
        print(f, {k: r["ops"].get(k, 0) for k in ("v_mad_i64_i32", "v_mad_u64_u32", "v_mul_lo_u32", "global_load_dwordx4")},
              "VALU", r["valu"], "registers", r["regs"], "scratch", r["scratch"])
    n = lambda r, k: r["ops"].get(k, 0)
    # the signed multiply-adds: all of the chain and of the four products of the way back, none more, none fewer
    assert n(new, "v_mad_i64_i32") == n(old, "v_mad_i64_i32") == n(mixed, "v_mad_i64_i32")
    # the two dropped fp28 products, counted from the old assembly
    dropped = n(old, "v_mad_u64_u32") - n(mixed, "v_mad_u64_u32")
    assert 0 < dropped <= 2 * 2 * 14 * 14
    assert n(new, "v_mad_u64_u32") == n(old, "v_mad_u64_u32") - dropped
    assert n(new, "v_mad_u64_u32") <= 40          # addressing only
    # the re-slicing at the one site of chain_add
    assert mixed["valu"] - new["valu"] >= 60, (mixed["valu"], new["valu"])
    # the gather: seven 16-byte loads of a slot instead of eight
    assert n(new, "global_load_dwordx4") == n(mixed, "global_load_dwordx4") - 1 == n(old, "global_load_dwordx4") - 1
    assert new["scratch"] == 0 and not any(k.startswith("scratch_") for k in new["ops"])
    assert new["regs"] <= 256


def kernel_text():
    """k_fbw_accum as msm.hip has it, with DigitParams, load_scalar and window_bits, in a translation unit of its own"""
    src = open(os.path.join(ROOT, "rust-kzg_amd", "csrc", "msm.hip")).read().split("\n")

    def block(first_line_has, last_line_has=None):
        a = next(i for i, ln in enumerate(src) if first_line_has in ln)
        b = a if last_line_has is None else next(i for i in range(a, len(src)) if last_line_has in src[i])
        e = next(i for i in range(b, len(src)) if src[i] == "}")
        return src[a:e + 1]

    return "\n".join(['#include "g1_30s.hip.h"', "using ff::u32;", "using ff::u64;", "using g1::Xyzz;", "using WidePt = g1s::WidePt30;",
                      "namespace cut {"] + block("struct DigitParams {", "u32 window_bits(const u32 s[8]") +
                     ["constexpr u32 FBW_SKIP = 0xffffffffu;"] + block("template <int SPL, bool GLV>") + ["}"]) + "\n"


def test_the_kernel_itself_keeps_two_waves_per_simd(tmp_path):
    import build as B
    if not os.path.exists(B.hipcc_path()):
        pytest.skip("no hipcc: " + B.hipcc_path())
    text = kernel_text()
    assert "k_fbw_accum(DigitParams P" in text and "g1s::chain_add" in text and "g1s::hold(pk)" in text

    def one(inst):
        tag = inst.replace(", ", "_")
        src = tmp_path / ("accum_%s.hip" % tag)
        src.write_text(text + "template __global__ void cut::k_fbw_accum<%s>(cut::DigitParams, const u32*, const WidePt*, Xyzz*, size_t);\n" % inst)
        asm = tmp_path / ("accum_%s.s" % tag)
        subprocess.check_call([B.hipcc_path()] + B.COMPILE_FLAGS + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "rust-kzg_amd", "csrc"),
                               str(src), "-o", str(asm)], stderr=subprocess.DEVNULL)
        t = asm.read_text()
        agpr = re.search(r"\.agpr_count:\s*(\d+)", t)
        return (int(re.search(r"\.vgpr_count:\s*(\d+)", t).group(1)), int(agpr.group(1)) if agpr else 0,
                int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", t).group(1)), len(re.findall(r"^\s+scratch_", t, re.M)))

    insts = ("8, true", "4, false")
    with ThreadPoolExecutor(2) as pool:
        for inst, (vgpr, agpr, private, scratch_ops) in zip(insts, pool.map(one, insts)):
            print("k_fbw_accum<%s>: %d registers (%d of them accumulation registers), %d bytes of scratch" % (inst, vgpr, agpr, private))
            assert vgpr <= 256 and private == 0 and scratch_ops == 0, inst
