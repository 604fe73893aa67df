// Test-only device harness for the lane-parallel arithmetic (fpw.hip.h, g1w.hip.h, g1grp.hip.h) and for the single-lane
// routines of g1_28.hip.h that consume what the wide code stores.  Never linked into the product; includes only headers
// of rust-kzg_amd/csrc and needs no library.  tests/test_lane_arith_gpu.py builds and runs it, tests/lane_model.py holds
// the cases and the checkers.
//
// stdin:  blocks of   <op> <ncases>   followed by ncases * nin hex words (nin fixed per op, table in main)
// stdout: per block   <op> <ncases>   followed by one line of nout hex words per case
// All cases of a block run in ONE kernel launch: one wave per case for the fpw / g1w ops, one group of G lanes per case
// for the grp / single-lane ops (64 / G different cases side by side in a wave).
//
// Layouts (u32 words):
//   wide register, input    4 rows x 14 limbs = 56 words (lanes 14 and 15 of every row are loaded with zero)
//   wide register, output   64 words, lane by lane: rows and lanes 14, 15 are checked by the caller, not assumed
//   point                   56 words, g1::Xyzz as in memory: x, y, zzz, zz
//   group result            per lane of the group 57 words: the returned flag, then the point
// The output buffer is filled with SENTINEL before the launch: a word an op does not write stays that.
//
// -DLANE_CHECK_PLANT_ERROR adds 1 to one limb of the result of case 1 of every block after the code under test has run
// (limb 5 of row 2 of the first result register; limb 5 of x on the last lane of the group): the checkers must see it.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "g1grp.hip.h"
#include "g1w.hip.h"

using ff::u32;
using g1::Xyzz;
using g1w::WPt;

namespace {
constexpr u32 SENTINEL = 0xA5A5A5A5u;
constexpr int PT = 56;          // words of a point
constexpr int WREG = 56;        // words of a wide register on input
constexpr int MAX_ADD_N = 5, MAX_STRIDE = 3, ADD_N_SLOTS = (MAX_ADD_N - 1) * MAX_STRIDE + 1;
constexpr int CHAIN_STEPS = 64, CHAIN_OPERANDS = 8, MAX_DBL_K = 64;
constexpr int STORE_GUARD = 8;  // sentinel words in front of and behind the slot g1w::store writes
constexpr int GRP_OUT = 1 + PT;

#if defined(LANE_CHECK_PLANT_ERROR)
#define PLANT_WAVE() \
    if (blockIdx.x == 1 && lane == 37) out[37] += 1;
#define PLANT_GRP(G) \
    if (g == 1 && r == (G)-1) o[1 + 5] += 1;
#else
#define PLANT_WAVE()
#define PLANT_GRP(G)
#endif

__device__ __forceinline__ u32 ld_wide(const u32* in, int reg, int lane) {
    const int i = lane & 15, row = lane >> 4;
    return i < fp28::L ? in[reg * WREG + row * fp28::L + i] : 0u;
}
__device__ __forceinline__ void put_point(u32* out, const WPt& p, int lane) {
    out[lane] = p.x;
    out[64 + lane] = p.y;
    out[128 + lane] = p.zzz;
    out[192 + lane] = p.zz;
}
__device__ __forceinline__ Xyzz ld_point(const u32* w) {
    Xyzz p;
#pragma unroll
    for (int i = 0; i < fp28::L; ++i) {
        p.x.v[i] = w[i];
        p.y.v[i] = w[fp28::L + i];
        p.zzz.v[i] = w[2 * fp28::L + i];
        p.zz.v[i] = w[3 * fp28::L + i];
    }
    return p;
}
__device__ __forceinline__ fp28::Fe ld_fe(const u32* w) {
    fp28::Fe a;
#pragma unroll
    for (int i = 0; i < fp28::L; ++i) a.v[i] = w[i];
    return a;
}
__device__ __forceinline__ void st_point(u32* w, const Xyzz& p) {
#pragma unroll
    for (int i = 0; i < fp28::L; ++i) {
        w[i] = p.x.v[i];
        w[fp28::L + i] = p.y.v[i];
        w[2 * fp28::L + i] = p.zzz.v[i];
        w[3 * fp28::L + i] = p.zz.v[i];
    }
}

// ---- one wave per case ----
#define WAVE_KERNEL(NAME)                                                                                        \
    __global__ void __launch_bounds__(64) NAME(const u32* __restrict__ in_all, u32* __restrict__ out_all, int nin, int nout)
#define WAVE_PROLOGUE                                       \
    const int lane = threadIdx.x;                           \
    const fpw::Lane lc = fpw::lane_consts(lane);            \
    const u32* in = in_all + (size_t)blockIdx.x * nin;      \
    u32* out = out_all + (size_t)blockIdx.x * nout;         \
    (void)lc;

#define FPW_UNARY(NAME, EXPR)                       \
    WAVE_KERNEL(NAME) {                             \
        WAVE_PROLOGUE                               \
        const u32 a = ld_wide(in, 0, lane);         \
        out[lane] = (EXPR);                         \
        PLANT_WAVE()                                \
    }
#define FPW_BINARY(NAME, EXPR)                      \
    WAVE_KERNEL(NAME) {                             \
        WAVE_PROLOGUE                               \
        const u32 a = ld_wide(in, 0, lane);         \
        const u32 b = ld_wide(in, 1, lane);         \
        out[lane] = (EXPR);                         \
        PLANT_WAVE()                                \
    }
FPW_UNARY(k_wnorm, fpw::wnorm(a, lc))
FPW_UNARY(k_wnorm_full, fpw::wnorm_full(a, lc))
FPW_UNARY(k_wsqr, fpw::wsqr(a, lc))
FPW_BINARY(k_waddn, fpw::waddn(a, b, lc))
FPW_BINARY(k_wsub16, fpw::wsub16(a, b, lc))
FPW_BINARY(k_wsub32, fpw::wsub32(a, b, lc))
FPW_BINARY(k_wmul4, fpw::wmul4(a, b, lc))

WAVE_KERNEL(k_wdbl) {
    WAVE_PROLOGUE
    u32 X = ld_wide(in, 0, lane), Y = ld_wide(in, 1, lane), Z = ld_wide(in, 2, lane);
    fpw::wdbl(X, Y, Z, lc, lane);
    out[lane] = X;
    out[64 + lane] = Y;
    out[128 + lane] = Z;
    PLANT_WAVE()
}
// in: one element (14 words); out: the wide register, then limb k of from_wide's result in every lane (14 x 64)
WAVE_KERNEL(k_wide_roundtrip) {
    __shared__ u32 sh[16];
    WAVE_PROLOGUE
    const fp28::Fe a = ld_fe(in);
    const u32 w = fpw::to_wide(a, sh, lane);
    out[lane] = w;
    const fp28::Fe r = fpw::from_wide(w, sh, lane);
#pragma unroll
    for (int k = 0; k < fp28::L; ++k) out[64 * (1 + k) + lane] = r.v[k];
    PLANT_WAVE()
}
// in: one wide register; out: the answer in every lane
WAVE_KERNEL(k_is_zero) {
    __shared__ u32 sh[16];
    WAVE_PROLOGUE
    const u32 a = ld_wide(in, 0, lane);
    out[lane] = g1w::is_zero_mod_p(a, sh, lane) ? 1u : 0u;
    PLANT_WAVE()
}
// in: a point; out: the four registers load gives (256), STORE_GUARD + 56 + STORE_GUARD words around the slot store
// writes, then to_single's point in every lane (64 x 56)
WAVE_KERNEL(k_load_store) {
    __shared__ u32 sh[16];
    WAVE_PROLOGUE
    const WPt p = g1w::load((const Xyzz*)in, lane);
    put_point(out, p, lane);
    g1w::store((Xyzz*)(out + 256 + STORE_GUARD), p, lc, lane);
    const Xyzz s = g1w::to_single(p, lc, sh, lane);
    st_point(out + 256 + 2 * STORE_GUARD + PT + lane * PT, s);
    PLANT_WAVE()
}
WAVE_KERNEL(k_dbl) {
    WAVE_PROLOGUE
    WPt acc = g1w::load((const Xyzz*)in, lane);
    g1w::dbl(acc, lc, lane);
    put_point(out, acc, lane);
    PLANT_WAVE()
}
WAVE_KERNEL(k_dadd) {
    __shared__ u32 sh[16];
    WAVE_PROLOGUE
    WPt acc = g1w::load((const Xyzz*)in, lane);
    const WPt b = g1w::load((const Xyzz*)(in + PT), lane);
    g1w::dadd(acc, b, lc, sh, lane);
    put_point(out, acc, lane);
    PLANT_WAVE()
}
// in: a point, k
WAVE_KERNEL(k_dbl_k) {
    WAVE_PROLOGUE
    WPt acc = g1w::load((const Xyzz*)in, lane);
    g1w::dbl_k(acc, (int)in[PT], lc, lane);
    put_point(out, acc, lane);
    PLANT_WAVE()
}
// in: the accumulator, n, stride, ADD_N_SLOTS points
WAVE_KERNEL(k_add_n) {
    __shared__ u32 sh[16];
    WAVE_PROLOGUE
    WPt acc = g1w::load((const Xyzz*)in, lane);
    g1w::add_n(acc, (const Xyzz*)(in + PT + 2), (size_t)in[PT + 1], (int)in[PT], lc, sh, lane);
    put_point(out, acc, lane);
    PLANT_WAVE()
}
// in: the accumulator, the number of steps, CHAIN_OPERANDS points, CHAIN_STEPS x (op, argument): op 0 = dbl, 1 = dadd of
// operand <argument>, 2 = dbl_k by <argument>; out: the four registers after every step
WAVE_KERNEL(k_chain) {
    __shared__ u32 sh[16];
    WAVE_PROLOGUE
    WPt acc = g1w::load((const Xyzz*)in, lane);
    const int steps = (int)in[PT];
    const u32* operands = in + PT + 1;
    const u32* script = operands + CHAIN_OPERANDS * PT;
#pragma unroll 1
    for (int s = 0; s < steps; ++s) {
        const u32 op = script[2 * s], arg = script[2 * s + 1];
        if (op == 0) g1w::dbl(acc, lc, lane);
        else if (op == 1) g1w::dadd(acc, g1w::load((const Xyzz*)(operands + arg * PT), lane), lc, sh, lane);
        else g1w::dbl_k(acc, (int)arg, lc, lane);
        put_point(out + s * 256, acc, lane);
    }
    PLANT_WAVE()
}

// ---- one group of G lanes per case ----
#define GRP_KERNEL(NAME) \
    __global__ void __launch_bounds__(64) NAME(const u32* __restrict__ in_all, u32* __restrict__ out_all, int nin, int ncases)
#define GRP_PROLOGUE(G)                                                   \
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;       \
    if (t >= (size_t)ncases * (G)) return;                                \
    const int r = (int)(t % (G));                                         \
    const size_t g = t / (G);                                             \
    const u32* in = in_all + g * nin;                                     \
    u32* o = out_all + t * GRP_OUT;

template <int G>
GRP_KERNEL(k_grp_dbl) {
    GRP_PROLOGUE(G)
    Xyzz acc = ld_point(in);
    grp::dbl_body<G>(acc, r);
    o[0] = 0;
    st_point(o + 1, acc);
    PLANT_GRP(G)
}
template <int G>
GRP_KERNEL(k_grp_dadd) {
    GRP_PROLOGUE(G)
    Xyzz acc = ld_point(in);
    const Xyzz b = ld_point(in + PT);
    o[0] = grp::dadd_body<G>(acc, b, r) ? 1u : 0u;
    st_point(o + 1, acc);
    PLANT_GRP(G)
}
// in: the accumulator, x2, y2
GRP_KERNEL(k_grp_madd4) {
    GRP_PROLOGUE(4)
    Xyzz acc = ld_point(in);
    grp::madd_body4(acc, ld_fe(in + PT), ld_fe(in + PT + fp28::L), r);
    o[0] = 0;
    st_point(o + 1, acc);
    PLANT_GRP(4)
}
// the single-lane routines of g1_28.hip.h on the device (the host build of the same text is checked on the CPU)
GRP_KERNEL(k_one_dadd) {
    GRP_PROLOGUE(1)
    Xyzz acc = ld_point(in);
    g1::dadd(acc, ld_point(in + PT));
    o[0] = 0;
    st_point(o + 1, acc);
    PLANT_GRP(1)
}
GRP_KERNEL(k_one_dadd_unequal) {
    GRP_PROLOGUE(1)
    Xyzz acc = ld_point(in);
    o[0] = g1::dadd_unequal(acc, ld_point(in + PT)) ? 1u : 0u;
    st_point(o + 1, acc);
    PLANT_GRP(1)
}
GRP_KERNEL(k_one_dbl_k) {
    GRP_PROLOGUE(1)
    Xyzz acc = ld_point(in);
    g1::dbl_k(acc, (int)in[PT]);
    o[0] = 0;
    st_point(o + 1, acc);
    PLANT_GRP(1)
}
GRP_KERNEL(k_one_madd) {
    GRP_PROLOGUE(1)
    Xyzz acc = ld_point(in);
    g1::madd(acc, ld_fe(in + PT), ld_fe(in + PT + fp28::L));
    o[0] = 0;
    st_point(o + 1, acc);
    PLANT_GRP(1)
}
// in: the accumulator, its chain state, x2, y2, the sign mask; out: the new chain state as the flag
GRP_KERNEL(k_one_chain_add) {
    GRP_PROLOGUE(1)
    Xyzz acc = ld_point(in);
    u32 st = in[PT];
    g1::chain_add(acc, st, ld_fe(in + PT + 1), ld_fe(in + PT + 1 + fp28::L), in[PT + 1 + 2 * fp28::L]);
    o[0] = st;
    st_point(o + 1, acc);
    PLANT_GRP(1)
}
GRP_KERNEL(k_one_reduce_xy) {
    GRP_PROLOGUE(1)
    Xyzz acc = ld_point(in);
    g1::reduce_xy(acc);
    o[0] = 0;
    st_point(o + 1, acc);
    PLANT_GRP(1)
}
// out: the three coordinates in blst layout (36 words) after the flag
GRP_KERNEL(k_one_to_blst) {
    GRP_PROLOGUE(1)
    const Xyzz acc = ld_point(in);
    ff::Fp j[3];
    g1::to_blst_jacobian(j, acc);
    o[0] = 0;
    for (int c = 0; c < 3; ++c)
        for (int i = 0; i < 12; ++i) o[1 + 12 * c + i] = j[c].v[i];
    PLANT_GRP(1)
}

typedef void (*Kernel)(const u32*, u32*, int, int);
struct Op {
    const char* name;
    Kernel kernel;
    int group;  // 0: one wave per case; G: one group of G lanes per case
    int nin, nout;
};
const Op OPS[] = {
    {"wnorm", k_wnorm, 0, WREG, 64},
    {"wnorm_full", k_wnorm_full, 0, WREG, 64},
    {"wsqr", k_wsqr, 0, WREG, 64},
    {"waddn", k_waddn, 0, 2 * WREG, 64},
    {"wsub16", k_wsub16, 0, 2 * WREG, 64},
    {"wsub32", k_wsub32, 0, 2 * WREG, 64},
    {"wmul4", k_wmul4, 0, 2 * WREG, 64},
    {"wdbl", k_wdbl, 0, 3 * WREG, 3 * 64},
    {"wide_roundtrip", k_wide_roundtrip, 0, fp28::L, 64 * (1 + fp28::L)},
    {"is_zero", k_is_zero, 0, WREG, 64},
    {"load_store", k_load_store, 0, PT, 256 + 2 * STORE_GUARD + PT + 64 * PT},
    {"dbl", k_dbl, 0, PT, 256},
    {"dadd", k_dadd, 0, 2 * PT, 256},
    {"dbl_k", k_dbl_k, 0, PT + 1, 256},
    {"add_n", k_add_n, 0, PT + 2 + ADD_N_SLOTS * PT, 256},
    {"chain", k_chain, 0, PT + 1 + CHAIN_OPERANDS * PT + 2 * CHAIN_STEPS, CHAIN_STEPS * 256},
    {"grp_dbl1", k_grp_dbl<1>, 1, PT, GRP_OUT},
    {"grp_dbl2", k_grp_dbl<2>, 2, PT, 2 * GRP_OUT},
    {"grp_dbl4", k_grp_dbl<4>, 4, PT, 4 * GRP_OUT},
    {"grp_dadd1", k_grp_dadd<1>, 1, 2 * PT, GRP_OUT},
    {"grp_dadd2", k_grp_dadd<2>, 2, 2 * PT, 2 * GRP_OUT},
    {"grp_dadd4", k_grp_dadd<4>, 4, 2 * PT, 4 * GRP_OUT},
    {"grp_madd4", k_grp_madd4, 4, PT + 2 * fp28::L, 4 * GRP_OUT},
    {"one_dadd", k_one_dadd, 1, 2 * PT, GRP_OUT},
    {"one_dadd_unequal", k_one_dadd_unequal, 1, 2 * PT, GRP_OUT},
    {"one_dbl_k", k_one_dbl_k, 1, PT + 1, GRP_OUT},
    {"one_madd", k_one_madd, 1, PT + 2 * fp28::L, GRP_OUT},
    {"one_chain_add", k_one_chain_add, 1, PT + 2 + 2 * fp28::L, GRP_OUT},
    {"one_to_blst", k_one_to_blst, 1, PT, GRP_OUT},
    {"one_reduce_xy", k_one_reduce_xy, 1, PT, GRP_OUT},
};

[[noreturn]] void fail(const std::string& what) {
    printf("lane_check error: %s\n", what.c_str());
    fflush(stdout);
    fprintf(stderr, "lane_check error: %s\n", what.c_str());
    exit(1);
}
#define HIP_OK(CALL)                                                                             \
    do {                                                                                         \
        const hipError_t e_ = (CALL);                                                            \
        if (e_ != hipSuccess) fail(std::string("HIP error: ") + hipGetErrorString(e_) + " in " #CALL); \
    } while (0)

// the header words an op uses as a count or an index: nothing out of range reaches a kernel
void validate(const Op& op, const u32* c, size_t k) {
    const std::string where = std::string(op.name) + " case " + std::to_string(k);
    if (!strcmp(op.name, "dbl_k") || !strcmp(op.name, "one_dbl_k")) {
        if (c[PT] > (u32)MAX_DBL_K) fail(where + ": k out of range");
    } else if (!strcmp(op.name, "add_n")) {
        if (c[PT] < 1 || c[PT] > (u32)MAX_ADD_N || c[PT + 1] < 1 || c[PT + 1] > (u32)MAX_STRIDE) fail(where + ": n or stride out of range");
    } else if (!strcmp(op.name, "chain")) {
        if (c[PT] > (u32)CHAIN_STEPS) fail(where + ": too many steps");
        const u32* script = c + PT + 1 + CHAIN_OPERANDS * PT;
        for (u32 s = 0; s < c[PT]; ++s) {
            const u32 o = script[2 * s], a = script[2 * s + 1];
            if (o > 2 || (o == 1 && a >= (u32)CHAIN_OPERANDS) || (o == 2 && a > (u32)MAX_DBL_K)) fail(where + ": bad step");
        }
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
        if (op->group == 0) {
            hipLaunchKernelGGL(op->kernel, dim3((unsigned)ncases), dim3(64), 0, 0, (const u32*)d_in, d_out, op->nin, op->nout);
        } else {
            const size_t threads = ncases * op->group;
            hipLaunchKernelGGL(op->kernel, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, 0, (const u32*)d_in, d_out, op->nin, (int)ncases);
        }
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
