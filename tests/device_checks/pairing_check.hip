// Test-only device harness for the pairing tower (fp12w.hip.h): every operation of the interpreter, the Miller loop and
// the final exponentiation on the device, one wave per case.  Never linked into the product; includes only headers of
// rust-kzg_amd/csrc and needs no library.  tests/test_pairing_arith_gpu.py builds and runs it, tests/pairing_model.py
// holds the cases and the checkers.  The text protocol is lane_check.hip's:
//
// stdin:  blocks of   <op> <ncases>   followed by ncases * nin hex words (nin fixed per op)
// stdout: per block   <op> <ncases>   followed by one line of nout hex words per case, then "done"
//
// unit     in:  8 program words | skip flag of pair 0, of pair 1 | slots 1, 2, 3 (192 words each: 12 coefficients x 16
//               words, words 14 and 15 zero) | per pair Z^3, X*Z, Y (16 words each) | per pair ONE line-table entry (64
//               words: the table of step 0) | the Frobenius constants (192 words)
//          out: the result REGISTERS of the last operation, coefficient by coefficient, all 64 lanes (12 x 64 words): the
//               four rows and lanes 14, 15 are checked by the caller, not assumed
// pairing  in:  a1, b1 (blst_p1: 36 words each) | table present flag of pair 0, of pair 1 | two line tables (68 x 64
//               words each) | the Frobenius constants | the program length | 768 program words
//          out: slot 0 after the program (192 words) | the verdict | the skip flag of pair 0, of pair 1
// winv     in:  one element (16 words, N-form, value < 50p); out: the result register of the Fp inversion, all 64 lanes
// The output buffer is filled with SENTINEL before the launch: a word an op does not write stays that.
//
// -DPAIRING_CHECK_PLANT_ERROR adds 1 to one limb of the result of case 1 of every block (limb 5 of row 2 of coefficient 3;
// limb 5 of coefficient 3 of slot 0): the checkers must see it.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fp12w.hip.h"

using ff::u32;

namespace {
constexpr u32 SENTINEL = 0xA5A5A5A5u;
constexpr int UNIT_PROG = 8;
constexpr int UNIT_SLOTS = UNIT_PROG + 2, UNIT_PAIRS = UNIT_SLOTS + 3 * fp12w::SLOT_WORDS,
              UNIT_LINES = UNIT_PAIRS + 2 * fp12w::PAIR_WORDS, UNIT_FROB = UNIT_LINES + 2 * fp12w::LINE_WORDS,
              UNIT_NIN = UNIT_FROB + fp12w::FROB_WORDS, UNIT_NOUT = 12 * 64;
constexpr int PAIRING_PROG = 768;
constexpr int PAIRING_TABS = 72 + 2, PAIRING_FROB = PAIRING_TABS + 2 * fp12w::TABLE_WORDS,
              PAIRING_NPROG = PAIRING_FROB + fp12w::FROB_WORDS, PAIRING_NIN = PAIRING_NPROG + 1 + PAIRING_PROG,
              PAIRING_NOUT = fp12w::SLOT_WORDS + 3;

__global__ void __launch_bounds__(64) k_unit(const u32* __restrict__ in_all, u32* __restrict__ out_all, int nin, int nout) {
    __shared__ u32 sh[fp12w::WAVE_WORDS];
    const int lane = threadIdx.x;
    const u32* in = in_all + (size_t)blockIdx.x * nin;
    u32* out = out_all + (size_t)blockIdx.x * nout;
    const fp12w::Ctx c = fp12w::make_ctx(lane);
    for (int k = lane; k < fp12w::WAVE_WORDS; k += 64) sh[k] = 0;
    fpw::wave_sync();
    for (int k = lane; k < 3 * fp12w::SLOT_WORDS; k += 64) sh[fp12w::SLOT_WORDS + k] = in[UNIT_SLOTS + k];
    for (int k = lane; k < 2 * fp12w::PAIR_WORDS; k += 64) fp12w::pair_words(sh, 0)[k] = in[UNIT_PAIRS + k];
    fpw::wave_sync();
    fp12w::Pairs pr;
    pr.tab[0] = in + UNIT_LINES;
    pr.tab[1] = in + UNIT_LINES + fp12w::LINE_WORDS;
    pr.skip[0] = in[UNIT_PROG] != 0;
    pr.skip[1] = in[UNIT_PROG + 1] != 0;
    fp12w::run_program<true>(in, UNIT_PROG, sh, pr, in + UNIT_FROB, c, out);
#if defined(PAIRING_CHECK_PLANT_ERROR)
    if (blockIdx.x == 1 && lane == 37) out[3 * 64 + 37] += 1;
#endif
}

__global__ void __launch_bounds__(64) k_pairing(const u32* __restrict__ in_all, u32* __restrict__ out_all, int nin, int nout) {
    __shared__ u32 sh[fp12w::WAVE_WORDS];
    const int lane = threadIdx.x;
    const u32* in = in_all + (size_t)blockIdx.x * nin;
    u32* out = out_all + (size_t)blockIdx.x * nout;
    const fp12w::Ctx c = fp12w::make_ctx(lane);
    for (int k = lane; k < fp12w::WAVE_WORDS; k += 64) sh[k] = 0;
    fpw::wave_sync();
    fp12w::Pairs pr;
    pr.tab[0] = in[72] ? in + PAIRING_TABS : nullptr;
    pr.tab[1] = in[73] ? in + PAIRING_TABS + fp12w::TABLE_WORDS : nullptr;
    fp12w::pairs_prepare(pr, sh, in, in + 36, c);
    fp12w::run_program<false>(in + PAIRING_NPROG + 1, (int)in[PAIRING_NPROG], sh, pr, in + PAIRING_FROB, c, nullptr);
    const bool one = fp12w::f12_is_one(fp12w::f12_load(sh, 0, c), c, fp12w::xchg_words(sh));
    for (int k = lane; k < fp12w::SLOT_WORDS; k += 64) out[k] = sh[k];
    if (lane == 0) {
        out[fp12w::SLOT_WORDS] = one ? 1u : 0u;
        out[fp12w::SLOT_WORDS + 1] = pr.skip[0] ? 1u : 0u;
        out[fp12w::SLOT_WORDS + 2] = pr.skip[1] ? 1u : 0u;
    }
#if defined(PAIRING_CHECK_PLANT_ERROR)
    if (blockIdx.x == 1 && lane == 0) out[3 * 16 + 5] += 1;
#endif
}

// in: one element (16 words); out: winv's result register, all 64 lanes
__global__ void __launch_bounds__(64) k_winv(const u32* __restrict__ in_all, u32* __restrict__ out_all, int nin, int nout) {
    const int lane = threadIdx.x;
    const fp12w::Ctx c = fp12w::make_ctx(lane);
    out_all[(size_t)blockIdx.x * nout + lane] = fp12w::winv(in_all[(size_t)blockIdx.x * nin + (lane & 15)], c);
#if defined(PAIRING_CHECK_PLANT_ERROR)
    if (blockIdx.x == 1 && lane == 37) out_all[(size_t)blockIdx.x * nout + 37] += 1;
#endif
}

typedef void (*Kernel)(const u32*, u32*, int, int);
struct Op {
    const char* name;
    Kernel kernel;
    int nin, nout;
};
const Op OPS[] = {
    {"unit", k_unit, UNIT_NIN, UNIT_NOUT},
    {"pairing", k_pairing, PAIRING_NIN, PAIRING_NOUT},
    {"winv", k_winv, 16, 64},
};

[[noreturn]] void fail(const std::string& what) {
    printf("pairing_check error: %s\n", what.c_str());
    fflush(stdout);
    fprintf(stderr, "pairing_check error: %s\n", what.c_str());
    exit(1);
}
#define HIP_OK(CALL)                                                                             \
    do {                                                                                         \
        const hipError_t e_ = (CALL);                                                            \
        if (e_ != hipSuccess) fail(std::string("HIP error: ") + hipGetErrorString(e_) + " in " #CALL); \
    } while (0)

// every program word names an operation the interpreter has, slots below NSLOTS and a table step that exists; every
// 16-word element has words 14 and 15 zero: nothing out of range reaches a kernel
void validate_program(const std::string& where, const u32* prog, u32 n, u32 steps) {
    for (u32 k = 0; k < n; ++k) {
        const u32 w = prog[k], op = w & 255u, d = (w >> 8) & 255u, a = (w >> 16) & 255u, b = w >> 24;
        if (op > fp12w::OP_LINE || d >= (u32)fp12w::NSLOTS || a >= (u32)fp12w::NSLOTS) fail(where + ": bad program word");
        if (op == fp12w::OP_MUL && b >= (u32)fp12w::NSLOTS) fail(where + ": bad second operand");
        if (op == fp12w::OP_LINE && b >= steps) fail(where + ": table step out of range");
    }
}
void validate_elements(const std::string& where, const u32* w, int nwords) {
    for (int k = 0; k < nwords; k += 16)
        if (w[k + 14] || w[k + 15]) fail(where + ": words 14, 15 of an element are not zero");
}
void validate(const Op& op, const u32* c, size_t k) {
    const std::string where = std::string(op.name) + " case " + std::to_string(k);
    if (!strcmp(op.name, "winv")) {
        validate_elements(where, c, 16);
    } else if (!strcmp(op.name, "unit")) {
        validate_program(where, c, UNIT_PROG, 1);
        validate_elements(where, c + UNIT_SLOTS, UNIT_NIN - UNIT_SLOTS);
    } else {
        if (c[PAIRING_NPROG] > (u32)PAIRING_PROG) fail(where + ": program too long");
        validate_program(where, c + PAIRING_NPROG + 1, c[PAIRING_NPROG], fp12w::LINE_STEPS);
        validate_elements(where, c + PAIRING_TABS, 2 * fp12w::TABLE_WORDS + fp12w::FROB_WORDS);
    }
}
}  // namespace

int main() {
    char name[64];
    unsigned long ncases;
    while (scanf("%63s %lu", name, &ncases) == 2) {
        const Op* op = nullptr;
        for (const Op& o : OPS)
            if (!strcmp(o.name, name)) op = &o;
        if (!op) fail(std::string("unknown op ") + name);
        if (ncases == 0 || ncases > 100000) fail("case count out of range");
        std::vector<u32> in((size_t)ncases * op->nin), out((size_t)ncases * op->nout, SENTINEL);
        for (u32& w : in)
            if (scanf("%x", &w) != 1) fail(std::string("short input for ") + name);
        for (size_t k = 0; k < ncases; ++k) validate(*op, in.data() + k * op->nin, k);
        u32 *d_in = nullptr, *d_out = nullptr;
        HIP_OK(hipMalloc((void**)&d_in, in.size() * sizeof(u32)));
        HIP_OK(hipMalloc((void**)&d_out, out.size() * sizeof(u32)));
        HIP_OK(hipMemcpy(d_in, in.data(), in.size() * sizeof(u32), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_out, out.data(), out.size() * sizeof(u32), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(op->kernel, dim3((unsigned)ncases), dim3(64), 0, 0, (const u32*)d_in, d_out, op->nin, op->nout);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.data(), d_out, out.size() * sizeof(u32), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_in));
        HIP_OK(hipFree(d_out));
        printf("%s %lu\n", name, ncases);
        std::string line;
        char buf[16];
        for (size_t k = 0; k < ncases; ++k) {
            line.clear();
            for (int i = 0; i < op->nout; ++i) {
                snprintf(buf, sizeof buf, "%x ", out[k * op->nout + i]);
                line += buf;
            }
            line += '\n';
            fputs(line.c_str(), stdout);
        }
    }
    printf("done\n");
    return 0;
}
