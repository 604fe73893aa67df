// Test-only harness for the Fp2 / G2 arithmetic that holds one value per lane (g2_28.hip.h, g2_io.hip.h,
// g2_lincomb.hip.h) and for the fp28.hip.h primitives under it.  Never linked into the product; includes only headers
// of rust-kzg_amd/csrc and needs no library.  tests/test_g2_arith_gpu.py builds and runs it for the device,
// tests/test_g2_device_cases_cpu.py cross-compiles it and runs its host form; tests/g2_lane_cases.py holds the cases
// and the checkers.
//
// stdin:  blocks of   <op> <ncases>   followed by ncases * nin hex words (nin fixed per op, table OPS)
// stdout: per block   <op> <ncases>   followed by one line of nout hex words per case, then `done`
// Device form: one __global__ __launch_bounds__(64) kernel PER OP, as every G2 kernel of the product is built; all
// cases of a block run in one launch, case i in lane i % 64 of workgroup i / 64, so the case list decides which cases
// share a wave.  Lanes at or beyond ncases return before they touch memory.  The two tree ops take one workgroup per
// case: the 64 slots in LDS, the levels ordered by fpw::wave_sync as setupcheck.hip's tree_sum orders them.
// Host form (-DG2_CHECK_HOST, any C++17 compiler with -x c++, no HIP): the same op bodies in a plain loop over cases.
// The output buffer is filled with SENTINEL before the launch: a word an op does not write stays that.
//
// Layouts (u32 words): Fe 14 limbs; F2 28 (c0, c1); Jac 84 (x, y, z); an affine point 56 (x, y); ff::Fp 12; ff::Fr 8;
// bytes one per word.
//
// -DG2_CHECK_PLANT_ERROR spoils the result of case 1 of every block after the code under test has run: 1 is added to
// one limb, or a verdict / one byte has its lowest bit flipped (the word and the kind are in the op's definition).
#if !defined(G2_CHECK_HOST)
#include <hip/hip_runtime.h>
#endif

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "g2_io.hip.h"
#include "g2_lincomb.hip.h"
#if !defined(G2_CHECK_HOST)
#include "fpw.hip.h"
#endif

using ff::u32;
using fp28::Fe;
using g2::F2;
using g2::Jac;

namespace {
constexpr u32 SENTINEL = 0xA5A5A5A5u;
constexpr int FE = 14, F2W = 28, JAC = 84, AFF = 56, FPW = 12;
#if defined(G2_CHECK_PLANT_ERROR)
constexpr bool PLANT = true;
#else
constexpr bool PLANT = false;
#endif

FF_HD Fe ld_fe(const u32* w) {
    Fe a;
#pragma unroll
    for (int i = 0; i < FE; ++i) a.v[i] = w[i];
    return a;
}
FF_HD F2 ld_f2(const u32* w) { return {ld_fe(w), ld_fe(w + FE)}; }
FF_HD Jac ld_jac(const u32* w) { return {ld_f2(w), ld_f2(w + F2W), ld_f2(w + 2 * F2W)}; }
FF_HD ff::Fp ld_fp(const u32* w) {
    ff::Fp a;
#pragma unroll
    for (int i = 0; i < FPW; ++i) a.v[i] = w[i];
    return a;
}
FF_HD void st(u32* w, const Fe& a) {
#pragma unroll
    for (int i = 0; i < FE; ++i) w[i] = a.v[i];
}
FF_HD void st(u32* w, const F2& a) {
    st(w, a.c0);
    st(w + FE, a.c1);
}
FF_HD void st(u32* w, const Jac& p) {
    st(w, p.x);
    st(w + F2W, p.y);
    st(w + 2 * F2W, p.z);
}
FF_HD void st(u32* w, const ff::Fp& a) {
#pragma unroll
    for (int i = 0; i < FPW; ++i) w[i] = a.v[i];
}

// ---- one case per lane: the body of an op, then its kernel (or its loop)
#if defined(G2_CHECK_HOST)
#define OP_RUNNER(NAME, NIN, NOUT, PWORD, PXOR)                                   \
    void k_##NAME(const u32* in_all, u32* out_all, u32 n) {                       \
        for (size_t i = 0; i < n; ++i) {                                          \
            u32* out = out_all + i * (NOUT);                                      \
            op_##NAME(in_all + i * (NIN), out);                                   \
            if (PLANT && i == 1) out[PWORD] = (PXOR) ? out[PWORD] ^ 1u : out[PWORD] + 1u; \
        }                                                                         \
    }
#else
#define OP_RUNNER(NAME, NIN, NOUT, PWORD, PXOR)                                                                        \
    __global__ void __launch_bounds__(64) k_##NAME(const u32* __restrict__ in_all, u32* __restrict__ out_all, u32 n) { \
        const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;                                                        \
        if (i >= n) return;                                                                                            \
        u32* out = out_all + i * (NOUT);                                                                               \
        op_##NAME(in_all + i * (NIN), out);                                                                            \
        if (PLANT && i == 1) out[PWORD] = (PXOR) ? out[PWORD] ^ 1u : out[PWORD] + 1u;                                  \
    }
#endif
// LANE_OP(name, words in, words out, the word a planted error spoils, 1: flip its lowest bit / 0: add 1) { body }
#define LANE_OP(NAME, NIN, NOUT, PWORD, PXOR, ...)                      \
    FF_HD void op_##NAME(const u32* in, u32* out) { __VA_ARGS__ }       \
    OP_RUNNER(NAME, NIN, NOUT, PWORD, PXOR)

// ---- fp28
LANE_OP(fp_mul, 2 * FE, FE, 5, 0, st(out, fp28::mul(ld_fe(in), ld_fe(in + FE)));)
LANE_OP(fp_sqr, FE, FE, 5, 0, st(out, fp28::sqr(ld_fe(in)));)
LANE_OP(fp_mul2, 4 * FE, FE, 5, 0, st(out, fp28::mul2_inline(ld_fe(in), ld_fe(in + FE), ld_fe(in + 2 * FE), ld_fe(in + 3 * FE)));)
#define FP_SUBS(K)                                                                               \
    LANE_OP(fp_sub##K, 2 * FE, FE, 5, 0, st(out, fp28::sub<K>(ld_fe(in), ld_fe(in + FE)));)      \
    LANE_OP(fp_subl##K, 2 * FE, FE, 5, 0, st(out, fp28::sub_lazy<K>(ld_fe(in), ld_fe(in + FE)));) \
    LANE_OP(fp_neg##K, FE, FE, 5, 0, st(out, fp28::neg<K>(ld_fe(in)));)
FP_SUBS(2)
FP_SUBS(4)
FP_SUBS(8)
FP_SUBS(16)
FP_SUBS(32)
// in: s, y, the sign mask
LANE_OP(fp_ssl8, 2 * FE + 1, FE, 5, 0, st(out, fp28::sub_signed_lazy<8>(ld_fe(in), ld_fe(in + FE), in[2 * FE]));)
LANE_OP(fp_ssl16, 2 * FE + 1, FE, 5, 0, st(out, fp28::sub_signed_lazy<16>(ld_fe(in), ld_fe(in + FE), in[2 * FE]));)
LANE_OP(fp_sub2bc, 3 * FE, FE, 5, 0, st(out, fp28::sub_2b_c(ld_fe(in), ld_fe(in + FE), ld_fe(in + 2 * FE)));)
LANE_OP(fp_norm, FE, FE, 5, 0, Fe a = ld_fe(in); fp28::norm(a); st(out, a);)
LANE_OP(fp_iszero, FE, 1, 0, 1, out[0] = fp28::is_zero_mod_p(ld_fe(in)) ? 1u : 0u;)
LANE_OP(fp_canon, FE, FE, 5, 0, st(out, fp28::canon(ld_fe(in)));)
LANE_OP(fp_from_blst, FPW, FE, 5, 0, st(out, fp28::from_blst(ld_fp(in)));)
LANE_OP(fp_to_blst, FE, FPW, 5, 0, st(out, fp28::to_blst(ld_fe(in)));)
LANE_OP(fp_pack, FE, FPW, 5, 0, st(out, fp28::pack(ld_fe(in)));)
LANE_OP(fp_unpack, FPW, FE, 5, 0, st(out, fp28::unpack(ld_fp(in)));)

// ---- Fp2
LANE_OP(f2_add, 2 * F2W, F2W, 5, 0, st(out, g2::add(ld_f2(in), ld_f2(in + F2W)));)
LANE_OP(f2_dbl, F2W, F2W, 5, 0, st(out, g2::dbl(ld_f2(in)));)
LANE_OP(f2_sub4, 2 * F2W, F2W, 5, 0, st(out, g2::sub<4>(ld_f2(in), ld_f2(in + F2W)));)
LANE_OP(f2_sub8, 2 * F2W, F2W, 5, 0, st(out, g2::sub<8>(ld_f2(in), ld_f2(in + F2W)));)
LANE_OP(f2_sub16, 2 * F2W, F2W, 5, 0, st(out, g2::sub<16>(ld_f2(in), ld_f2(in + F2W)));)
LANE_OP(f2_sub32, 2 * F2W, F2W, 5, 0, st(out, g2::sub<32>(ld_f2(in), ld_f2(in + F2W)));)
LANE_OP(f2_neg2, F2W, F2W, 5, 0, st(out, g2::neg<2>(ld_f2(in)));)
LANE_OP(f2_neg16, F2W, F2W, 5, 0, st(out, g2::neg<16>(ld_f2(in)));)
LANE_OP(f2_mul, 2 * F2W, F2W, 5, 0, st(out, g2::mul(ld_f2(in), ld_f2(in + F2W)));)
LANE_OP(f2_sqr, F2W, F2W, 5, 0, st(out, g2::sqr(ld_f2(in)));)
LANE_OP(f2_mulfe, F2W + FE, F2W, 5, 0, st(out, g2::mul_fe(ld_f2(in), ld_fe(in + F2W)));)
LANE_OP(f2_red, F2W, F2W, 5, 0, st(out, g2::red(ld_f2(in)));)
LANE_OP(f2_inv, F2W, F2W, 5, 0, st(out, g2::inv(ld_f2(in)));)
LANE_OP(f2_iszero, F2W, 1, 0, 1, out[0] = g2::is_zero(ld_f2(in)) ? 1u : 0u;)

// ---- G2 points
LANE_OP(g2_dbl, JAC, JAC, 5, 0, Jac p = ld_jac(in); g2::dbl(p); st(out, p);)
// in: P, x2, y2; out: the returned state, then P as madd left it
LANE_OP(g2_madd, JAC + AFF, 1 + JAC, 1 + 5, 0, Jac p = ld_jac(in); out[0] = g2::madd(p, ld_f2(in + JAC), ld_f2(in + JAC + F2W)); st(out + 1, p);)
LANE_OP(g2_maddc, JAC + AFF, JAC, 5, 0, Jac p = ld_jac(in); g2::madd_complete(p, ld_f2(in + JAC), ld_f2(in + JAC + F2W)); st(out, p);)
// in: P, the entry's x, y, its flags, the sign mask
LANE_OP(g2_maddtab, JAC + AFF + 2, JAC, 5, 0,
        Jac p = ld_jac(in);
        g2::AffPt e;
        e.x = ld_f2(in + JAC);
        e.y = ld_f2(in + JAC + F2W);
        e.flags = in[JAC + AFF];
        e.pad[0] = e.pad[1] = e.pad[2] = 0;
        g2::madd_tab(p, e, in[JAC + AFF + 1]);
        st(out, p);)
LANE_OP(g2_add, 2 * JAC, JAC, 5, 0, Jac p = ld_jac(in); g2::add(p, ld_jac(in + JAC)); st(out, p);)
// in: P, Q, an affine R; out: add of every ordered pair of dbl(P), madd_complete(P, R), add(P, Q) (nine), then the
// doubling and the mixed addition of R of each (three pairs): 15 points, each routine's output into each routine
LANE_OP(g2_fedback, 2 * JAC + AFF, 15 * JAC, 5, 0,
        const Jac p = ld_jac(in);
        const F2 x2 = ld_f2(in + 2 * JAC);
        const F2 y2 = ld_f2(in + 2 * JAC + F2W);
        Jac o[3];
        o[0] = p;
        g2::dbl(o[0]);
        o[1] = p;
        g2::madd_complete(o[1], x2, y2);
        o[2] = p;
        g2::add(o[2], ld_jac(in + JAC));
        int at = 0;
        _Pragma("unroll 1") for (int i = 0; i < 3; ++i)
            _Pragma("unroll 1") for (int j = 0; j < 3; ++j) {
                Jac r = o[i];
                g2::add(r, o[j]);
                st(out + JAC * at++, r);
            }
        _Pragma("unroll 1") for (int i = 0; i < 3; ++i) {
            Jac r = o[i];
            g2::dbl(r);
            st(out + JAC * at++, r);
            r = o[i];
            g2::madd_complete(r, x2, y2);
            st(out + JAC * at++, r);
        })
// out: x, y, flags
LANE_OP(g2_toaff, JAC, AFF + 1, 5, 0, g2::AffPt a; g2::to_affine(a, ld_jac(in)); st(out, a.x); st(out + F2W, a.y); out[AFF] = a.flags;)
// in: a blst_p2 (six Fp)
LANE_OP(g2_fromblst, 6 * FPW, JAC, 5, 0,
        ff::Fp c[6];
        for (int k = 0; k < 6; ++k) c[k] = ld_fp(in + FPW * k);
        Jac p;
        g2::from_blst_jacobian(p, c);
        st(out, p);)
LANE_OP(g2_toblst, JAC, 6 * FPW, 5, 0,
        ff::Fp c[6];
        g2::to_blst_jacobian(c, ld_jac(in));
        for (int k = 0; k < 6; ++k) st(out + FPW * k, c[k]);)

// ---- g2io
LANE_OP(io_canon2, FE, FE, 5, 0, st(out, g2io::canon2(ld_fe(in)));)
LANE_OP(io_lex, F2W, 1, 0, 1, out[0] = g2io::lex_largest(ld_f2(in)) ? 1u : 0u;)
// out: the verdict, the root
LANE_OP(io_sqrt, F2W, 1 + F2W, 0, 1, F2 r; out[0] = g2io::sqrt(r, ld_f2(in)) ? 1u : 0u; st(out + 1, r);)
// in: 96 bytes; out: the verdict, flags, x, y
LANE_OP(io_uncompress, 96, 2 + AFF, 0, 1,
        unsigned char b[96];
        for (int k = 0; k < 96; ++k) b[k] = (unsigned char)in[k];
        g2::AffPt a;
        out[0] = g2io::uncompress(a, b) ? 1u : 0u;
        out[1] = a.flags;
        st(out + 2, a.x);
        st(out + 2 + F2W, a.y);)
LANE_OP(io_compress, JAC, 96, 50, 1,
        unsigned char b[96];
        g2io::compress(b, ld_jac(in));
        for (int k = 0; k < 96; ++k) out[k] = b[k];)
LANE_OP(io_psi, AFF, AFF, 5, 0, F2 px; F2 py; g2io::psi(px, py, ld_f2(in), ld_f2(in + F2W)); st(out, px); st(out + F2W, py);)
// in: x, y, flags
LANE_OP(io_ing2, AFF + 1, 1, 0, 1,
        g2::AffPt a;
        a.x = ld_f2(in);
        a.y = ld_f2(in + F2W);
        a.flags = in[AFF];
        a.pad[0] = a.pad[1] = a.pad[2] = 0;
        out[0] = g2io::in_g2(a) ? 1u : 0u;)
// in: one word, not read; out: psi_x(), psi_y() as this build holds them
LANE_OP(io_psiconst, 1, 2 * F2W, 5 + FE, 0, (void)in; st(out, g2io::psi_x()); st(out + F2W, g2io::psi_y());)

// ---- g2lc
// in: a blst_p2, a Montgomery blst_fr
LANE_OP(lc_term, 6 * FPW + 8, JAC, 5, 0,
        ff::Fp c[6];
        for (int k = 0; k < 6; ++k) c[k] = ld_fp(in + FPW * k);
        ff::Fr s;
        for (int k = 0; k < 8; ++k) s.v[k] = in[6 * FPW + k];
        Jac acc;
        g2lc::term(acc, c, s);
        st(out, acc);)

// the tree over 64 slots, one workgroup (one wave) per case.  LEVELS = 1: the level half = 32 alone, out the 32 slots it
// wrote; LEVELS = 6: all of tree_sum, out slot 0
constexpr int LANES = g2lc::LANES;
template <int LEVELS>
#if defined(G2_CHECK_HOST)
void k_lc_tree(const u32* in_all, u32* out_all, u32 n) {
    constexpr int KEEP = LEVELS == 1 ? LANES / 2 : 1;
    std::vector<Jac> slots(LANES);
    for (size_t c = 0; c < n; ++c) {
        for (int t = 0; t < LANES; ++t) slots[t] = ld_jac(in_all + (c * LANES + t) * JAC);
        int half = LANES / 2;
        for (int l = 0; l < LEVELS; ++l, half >>= 1)
            for (int t = 0; t < half; ++t) g2lc::tree_step(slots.data(), t, half);
        for (int t = 0; t < KEEP; ++t) st(out_all + (c * KEEP + t) * JAC, slots[t]);
        if (PLANT && c == 1) out_all[c * KEEP * JAC + 5] += 1;
    }
}
#else
__global__ void __launch_bounds__(64) k_lc_tree(const u32* __restrict__ in_all, u32* __restrict__ out_all, u32 n) {
    constexpr int KEEP = LEVELS == 1 ? LANES / 2 : 1;
    __shared__ Jac slots[LANES];
    const int t = threadIdx.x;
    const size_t c = blockIdx.x;
    if (c >= n) return;  // the whole workgroup
    slots[t] = ld_jac(in_all + (c * LANES + t) * JAC);
    fpw::wave_sync();
    int half = LANES / 2;
#pragma unroll 1
    for (int l = 0; l < LEVELS; ++l, half >>= 1) {
        if (t < half) g2lc::tree_step(slots, t, half);
        fpw::wave_sync();
    }
    if (t < KEEP) st(out_all + (c * KEEP + t) * JAC, slots[t]);
    if (PLANT && c == 1 && t == 0) out_all[c * KEEP * JAC + 5] += 1;
}
#endif

typedef void (*Runner)(const u32*, u32*, u32);
struct Op {
    const char* name;
    Runner run;
    int per_group;  // 0: one case per lane; 1: one workgroup per case
    int nin, nout;
};
#define ROW(NAME, NIN, NOUT) {#NAME, k_##NAME, 0, NIN, NOUT}
#define ROWS_SUBS(K) ROW(fp_sub##K, 2 * FE, FE), ROW(fp_subl##K, 2 * FE, FE), ROW(fp_neg##K, FE, FE)
const Op OPS[] = {
    ROW(fp_mul, 2 * FE, FE), ROW(fp_sqr, FE, FE), ROW(fp_mul2, 4 * FE, FE),
    ROWS_SUBS(2), ROWS_SUBS(4), ROWS_SUBS(8), ROWS_SUBS(16), ROWS_SUBS(32),
    ROW(fp_ssl8, 2 * FE + 1, FE), ROW(fp_ssl16, 2 * FE + 1, FE), ROW(fp_sub2bc, 3 * FE, FE), ROW(fp_norm, FE, FE),
    ROW(fp_iszero, FE, 1), ROW(fp_canon, FE, FE), ROW(fp_from_blst, FPW, FE), ROW(fp_to_blst, FE, FPW),
    ROW(fp_pack, FE, FPW), ROW(fp_unpack, FPW, FE),
    ROW(f2_add, 2 * F2W, F2W), ROW(f2_dbl, F2W, F2W), ROW(f2_sub4, 2 * F2W, F2W), ROW(f2_sub8, 2 * F2W, F2W),
    ROW(f2_sub16, 2 * F2W, F2W), ROW(f2_sub32, 2 * F2W, F2W), ROW(f2_neg2, F2W, F2W), ROW(f2_neg16, F2W, F2W),
    ROW(f2_mul, 2 * F2W, F2W), ROW(f2_sqr, F2W, F2W), ROW(f2_mulfe, F2W + FE, F2W), ROW(f2_red, F2W, F2W),
    ROW(f2_inv, F2W, F2W), ROW(f2_iszero, F2W, 1),
    ROW(g2_dbl, JAC, JAC), ROW(g2_madd, JAC + AFF, 1 + JAC), ROW(g2_maddc, JAC + AFF, JAC),
    ROW(g2_maddtab, JAC + AFF + 2, JAC), ROW(g2_add, 2 * JAC, JAC), ROW(g2_fedback, 2 * JAC + AFF, 15 * JAC),
    ROW(g2_toaff, JAC, AFF + 1), ROW(g2_fromblst, 6 * FPW, JAC), ROW(g2_toblst, JAC, 6 * FPW),
    ROW(io_canon2, FE, FE), ROW(io_lex, F2W, 1), ROW(io_sqrt, F2W, 1 + F2W), ROW(io_uncompress, 96, 2 + AFF),
    ROW(io_compress, JAC, 96), ROW(io_psi, AFF, AFF), ROW(io_ing2, AFF + 1, 1), ROW(io_psiconst, 1, 2 * F2W),
    ROW(lc_term, 6 * FPW + 8, JAC),
    {"lc_tree1", k_lc_tree<1>, 1, LANES * JAC, (LANES / 2) * JAC},
    {"lc_tree6", k_lc_tree<6>, 1, LANES * JAC, JAC},
};

[[noreturn]] void fail(const std::string& what) {
    printf("g2_check error: %s\n", what.c_str());
    fflush(stdout);
    fprintf(stderr, "g2_check error: %s\n", what.c_str());
    exit(1);
}

#if defined(G2_CHECK_HOST)
void run_op(const Op& op, const std::vector<u32>& in, std::vector<u32>& out, size_t n) { op.run(in.data(), out.data(), (u32)n); }
#else
#define HIP_OK(CALL)                                                                                   \
    do {                                                                                               \
        const hipError_t e_ = (CALL);                                                                  \
        if (e_ != hipSuccess) fail(std::string("HIP error: ") + hipGetErrorString(e_) + " in " #CALL); \
    } while (0)
void run_op(const Op& op, const std::vector<u32>& in, std::vector<u32>& out, size_t n) {
    u32 *d_in = nullptr, *d_out = nullptr;
    HIP_OK(hipMalloc((void**)&d_in, in.size() * sizeof(u32)));
    HIP_OK(hipMalloc((void**)&d_out, out.size() * sizeof(u32)));
    HIP_OK(hipMemcpy(d_in, in.data(), in.size() * sizeof(u32), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_out, out.data(), out.size() * sizeof(u32), hipMemcpyHostToDevice));
    const unsigned groups = op.per_group ? (unsigned)n : (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL(op.run, dim3(groups), dim3(64), 0, 0, (const u32*)d_in, d_out, (u32)n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out.data(), d_out, out.size() * sizeof(u32), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));
}
#endif
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
        run_op(*op, in, out, ncases);
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
