// Batched polynomial arithmetic over Fr: the reference's Poly<Fr> (blst/src/types/poly.rs: eval, scale / unscale,
// mul_direct, mul_fft, mul, inverse, long_div, fast_div, div) and FFTSettingsPoly::poly_mul_fft, npoly independent
// problems of one shape per call.  Every result is a field element with one value, so every route below gives the
// reference's elements exactly.  Nothing is serial in the polynomial's length: a dependent Fr multiplication is
// ~1.1 us on a lone wave (profiles/NOTES.md).
//
//   eval     one lane per (polynomial, x, chunk of CHUNK coefficients) runs Horner on its chunk; the partial sums are
//            combined with the powers of x^CHUNK — the recurrence H_m = S_m + C H_{m+1} of kzg.hip (frscan.hip.h),
//            inside a wave by the log-step scan, across waves through one summary each (k_poly_eval, then
//            k_poly_eval_carry when a polynomial has more than 64 chunks).  It is the n = 1 remainder of kzg.hip
//            without the replay and without a quotient.  2 or 3 launches per slice, k_kzg_pows included.
//   scale    one lane per coefficient, 5^-(i+1) or 5^(i+1) by square-and-multiply on the public exponent.  1 launch.
//   mul      direct form: one lane per (polynomial, output coefficient) takes its dot product; any shape.  1 launch.
//            transform form: k_poly_pad writes both operands of every polynomial, cut to out_len, zero-padded to N =
//            next_pow2(la' + lb' - 1), into one buffer; one forward transform of 2 npoly lists; k_poly_pointwise; one
//            inverse transform of npoly lists; k_poly_cut.  3 launches and 3 npoly transforms.
//            form 0 takes the direct form up to MUL_DIRECT_MAX multiplications per lane (the reference's rule "an
//            operand shorter than 64", poly.rs:399).
//   inverse  k_poly_inv0 inverts b[0] of the whole batch and raises the "b[0] == 0" flag.  The first INV_DIRECT_MAX
//            coefficients come from c_j = -c_0 sum_{i >= 1} b_i c_{j-i} in one launch, a wave per polynomial: lane i
//            keeps b_i and c_i, the dot product is spread over the lanes and summed by shuffles.  Then Newton's
//            c <- c (2 - b c) along the reference's precision sequence d <- 2d + bit (poly.rs:118-122), so the last
//            step lands on out_len: b mod x^(d+1) and c are transformed once at N = next_pow2((d+1) + 2 len(c) - 2),
//            k_poly_newton multiplies c (2 - b c) pointwise, one inverse transform, cut to d + 1 — 3 transforms and
//            3 launches a step, N <= next_pow2(2 out_len - 1).
//   div      lb == 1: one inversion per polynomial and a pointwise product.  Otherwise fast_div for every divisor
//            length (long_div would be a serial recurrence in the quotient's length; the quotient is the same):
//            the inverse of the flipped divisor to L = la - lb + 1, one product with the flipped dividend cut to L,
//            flipped on the way out.  The flips are index maps of the kernels that read and write (Operand), not
//            passes.  The "highest coefficient is zero" test is k_poly_inv0's flag.
// Wave-local exchange and global memory between launches only: no workgroup barrier in this file.  Everything between
// the upload and the download is enqueued on the handle's one stream; buffers stay device-resident; a call holds the
// handle's lock, runs in slices of polynomials when its workspace would take more than a share of the free HBM, and
// synchronises before it returns.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/kzg_mi355x.h"
#include "config.h"
#include "device_guard.h"
#include "ff.hip.h"
#include "fr29.hip.h"
#include "frscan.hip.h"
#include "ntt_internal.h"
#include "poly_internal.h"

using ff::Fr;
using ff::u32;
using namespace kzgamd_poly;

namespace {

constexpr size_t MUL_DIRECT_MAX = 63;  // multiplications per lane up to which form 0 takes the direct product
constexpr size_t INV_DIRECT_MAX = 64;  // coefficients of an inverse the one-wave recurrence computes: a lane each

// a polynomial of a batch as a kernel reads it: coefficient i of polynomial `poly`, flipped or not
struct Operand {
    const Fr* p;
    size_t len, stride;
    int flip;
};
__device__ __forceinline__ Fr op_at(const Operand& o, size_t poly, size_t i) {
    return o.p[poly * o.stride + (o.flip ? o.len - 1 - i : i)];
}

struct EvalShape {
    size_t len, nx, nseq;  // nseq = polynomials of the slice x nx: sequence = poly * nx + x index
    size_t M;              // chunks per polynomial
    u32 gw, wv;            // lanes of a wave per sequence (a power of two <= 64), waves per sequence (gw == 64 if > 1)
};

// thread = (sequence, chunk m), gw * wv slots per sequence.  Writes p(x) when a sequence fits one wave, otherwise the
// summary of every wave, sum_d C^d S_{64 w + d}, to sums[seq * wv + w].
__global__ void __launch_bounds__(256) k_poly_eval(Fr* __restrict__ ys, Fr* __restrict__ sums, const Fr* __restrict__ polys,
                                                   const Fr* __restrict__ pw, EvalShape s) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t slots = (size_t)s.gw * s.wv;
    const size_t seq = t / slots, m = t % slots;
    const bool live = seq < s.nseq && m < s.M;  // dead lanes carry zeros through the scan: no lane leaves early
    const Fr* p = polys + (live ? seq / s.nx : 0) * s.len;
    const Fr* mypw = pw + (live ? seq % s.nx : 0) * PW;
    const Fr x = mypw[0];
    Fr S = Fr::zero();
    if (live) {
        for (int i = CHUNK - 1; i >= 0; --i) {
            const size_t j = m * CHUNK + i;
            if (j < s.len) S = ff::add(p[j], fr_mul(x, S));
        }
    }
    const u32 lg = (u32)(m & (s.gw - 1));
    const Fr H = scan_suffix(S, lg, s.gw, mypw + 1);
    if (!live || lg != 0) return;
    if (s.wv == 1) ys[seq] = H;
    else sums[seq * s.wv + m / 64] = H;
}

// the summaries of the waves of a sequence -> p(x), G_w = W_w + C^64 G_{w+1}: a wave per sequence, a lane per summary,
// blocks of 64 summaries from the top
__global__ void __launch_bounds__(64) k_poly_eval_carry(Fr* __restrict__ ys, const Fr* __restrict__ sums, const Fr* __restrict__ pw,
                                                        EvalShape s) {
    const size_t seq = blockIdx.x;  // < nseq
    const u32 lane = threadIdx.x;
    const Fr* mypw = pw + (seq % s.nx) * PW + 7;  // (C^64)^(2^k), k = 0 .. 5
    const Fr* g = sums + seq * s.wv;
    Fr above = Fr::zero();
    for (size_t blk = ((size_t)s.wv + 63) / 64; blk-- > 0;) {
        const size_t w = blk * 64 + lane;
        Fr H = w < s.wv ? g[w] : Fr::zero();
        if (lane == 63) H = ff::add(H, fr_mul(mypw[0], above));
        H = scan_suffix(H, lane, 64, mypw);
        above = shfl_idx(H, 0);
    }
    if (lane == 0) ys[seq] = above;
}

// out[i] = in[i] * f^(i mod len + 1)
__global__ void __launch_bounds__(256) k_poly_scale(Fr* __restrict__ out, const Fr* __restrict__ in, Fr f, size_t len, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    out[t] = fr_mul(in[t], fr_pow(f, t % len + 1));
}

// thread = (polynomial, output coefficient i): sum_j a_j b_{i-j}
__global__ void __launch_bounds__(256) k_poly_mul_direct(Fr* __restrict__ out, size_t out_len, int out_flip, Operand a, Operand b,
                                                         size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t p = t / out_len, i = t % out_len;
    Fr acc = Fr::zero();
    if (i < a.len + b.len - 1) {
        const size_t j1 = i < a.len ? i : a.len - 1;
        for (size_t j = i >= b.len ? i - b.len + 1 : 0; j <= j1; ++j) acc = ff::add(acc, fr_mul(op_at(a, p, j), op_at(b, p, i - j)));
    }
    out[p * out_len + (out_flip ? out_len - 1 - i : i)] = acc;
}

// dst[(2 poly) N + i] = a_i (i < la), dst[(2 poly + 1) N + i] = b_i (i < lb), zeros up to N
__global__ void __launch_bounds__(256) k_poly_pad(Fr* __restrict__ dst, Operand a, size_t la, Operand b, size_t lb, size_t N,
                                                  size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t p = t / (2 * N), r = t % (2 * N);
    Fr v = Fr::zero();
    if (r < N) {
        if (r < la) v = op_at(a, p, r);
    } else if (r - N < lb) {
        v = op_at(b, p, r - N);
    }
    dst[t] = v;
}

// dst[poly N + i] = A_i B_i (NEWTON: C_i (2 - B_i C_i)) of the transformed pairs src[(2 poly) N + i], src[(2 poly + 1) N + i]
template <bool NEWTON>
__global__ void __launch_bounds__(256) k_poly_pointwise(Fr* __restrict__ dst, const Fr* __restrict__ src, size_t N, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t p = t / N, i = t % N;
    const Fr A = src[2 * p * N + i], B = src[(2 * p + 1) * N + i];
    if (NEWTON) {
        const Fr two = ff::add(Fr::one(), Fr::one());
        dst[t] = fr_mul(B, ff::sub(two, fr_mul(A, B)));
    } else {
        dst[t] = fr_mul(A, B);
    }
}

// out[poly out_stride + i] = src[poly N + i], i < out_len, zero beyond N
__global__ void __launch_bounds__(256) k_poly_cut(Fr* __restrict__ out, size_t out_stride, size_t out_len, int out_flip,
                                                  const Fr* __restrict__ src, size_t N, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t p = t / out_len, i = t % out_len;
    out[p * out_stride + (out_flip ? out_len - 1 - i : i)] = i < N ? src[p * N + i] : Fr::zero();
}

// out[poly out_stride] = 1 / b_poly[0]; a zero there raises the flag
__global__ void __launch_bounds__(64) k_poly_inv0(Fr* __restrict__ out, size_t out_stride, Operand b, int* __restrict__ flag, size_t npoly) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npoly) return;
    const Fr v = op_at(b, t, 0);
    if (v.is_zero()) {
        *flag = 1;
        out[t * out_stride] = v;
    } else {
        out[t * out_stride] = ff::inverse_bgcd(v);
    }
}

// a wave per polynomial: c_j = -c_0 sum_{i = 1 .. j} b_i c_{j-i}, j < D0 <= 64; lane i keeps b_i and c_i
__global__ void __launch_bounds__(64) k_poly_inv_direct(Fr* __restrict__ c, size_t stride, Operand b, size_t D0) {
    const size_t p = blockIdx.x;
    const u32 lane = threadIdx.x;
    const Fr c0 = c[p * stride];
    const Fr nc0 = ff::neg(c0);
    const Fr bl = lane >= 1 && lane < b.len && lane < D0 ? op_at(b, p, lane) : Fr::zero();
    Fr cl = lane == 0 ? c0 : Fr::zero();
    for (u32 j = 1; j < D0; ++j) {
        const Fr v = shfl_idx(cl, (int)((j - lane) & 63));  // c_{j - lane} where 1 <= lane <= j
        Fr term = fr_mul(bl, v);
        if (lane < 1 || lane > j) term = Fr::zero();
        for (int k = 32; k >= 1; k >>= 1) term = ff::add(term, shfl_xor(term, k));
        const Fr cj = fr_mul(nc0, term);
        if (lane == j) cl = cj;
    }
    if (lane < D0) c[p * stride + lane] = cl;
}

// q[i] = a[i] * inv[i / la]
__global__ void __launch_bounds__(256) k_poly_mul_const(Fr* __restrict__ q, const Fr* __restrict__ a, const Fr* __restrict__ inv, size_t la,
                                                        size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < total) q[t] = fr_mul(a[t], inv[t / la]);
}

// the transform a product by transforms runs; 0: none (an empty operand or output, or a product of two constants)
size_t mul_transform_len(size_t la, size_t lb, size_t out_len) {
    if (!la || !lb || !out_len) return 0;
    const size_t n = min_sz(la, out_len) + min_sz(lb, out_len) - 1;
    return n < 2 ? 0 : next_pow2(n);
}
bool mul_is_direct(size_t la, size_t lb, size_t out_len, int form) {
    if (form == 1 || mul_transform_len(la, lb, out_len) == 0) return true;
    if (form == 2) return false;
    return min_sz(min_sz(la, out_len), min_sz(lb, out_len)) <= MUL_DIRECT_MAX;
}

// the steps of an inverse to L coefficients: D0 of them by the recurrence, then Newton steps from m to n1 coefficients
struct InvStep {
    size_t m, n1, nb, N;  // nb = coefficients of b the step reads, N = its transform length
};
struct InvPlan {
    size_t D0 = 1, maxN = 0;
    std::vector<InvStep> steps;
};
InvPlan inv_plan(size_t lb, size_t L) {
    InvPlan pl;
    if (lb <= 1 || L <= 1) return pl;
    const size_t maxd = L - 1;
    size_t d = 0, mask = 1, prev = 1;
    while ((mask << 1) && (mask << 1) <= maxd) mask <<= 1;
    for (; mask; mask >>= 1) {
        d = 2 * d + ((maxd & mask) != 0);
        const size_t n1 = d + 1;
        if (n1 <= INV_DIRECT_MAX) {
            pl.D0 = n1;
        } else {
            InvStep s;
            s.m = prev;
            s.n1 = n1;
            s.nb = min_sz(lb, n1);
            s.N = next_pow2(s.nb + 2 * s.m - 2);
            if (s.N > pl.maxN) pl.maxN = s.N;
            pl.steps.push_back(s);
        }
        prev = n1;
    }
    return pl;
}
size_t div_transform_len(size_t la, size_t lb) {
    if (lb <= 1 || la < lb) return 0;
    const size_t L = la - lb + 1;
    size_t n = inv_plan(lb, L).maxN;
    if (!mul_is_direct(la, L, L, 0) && mul_transform_len(la, L, L) > n) n = mul_transform_len(la, L, L);
    return n;
}

// out[poly out_len + i] = coefficient i of a_poly b_poly (pc->f and pc->g hold 2 npoly N elements when not direct)
void enqueue_mul(PolyCtx* pc, Fr* out, size_t out_len, int out_flip, const Operand& a, const Operand& b, size_t npoly, int form) {
    hipStream_t st = pc->st;
    if (mul_is_direct(a.len, b.len, out_len, form)) {
        hipLaunchKernelGGL(k_poly_mul_direct, dim3(blocks(npoly * out_len)), dim3(256), 0, st, out, out_len, out_flip, a, b, npoly * out_len);
    } else {
        const size_t N = mul_transform_len(a.len, b.len, out_len);
        Fr *f = pc->f.as<Fr>(), *g = pc->g.as<Fr>();
        hipLaunchKernelGGL(k_poly_pad, dim3(blocks(2 * npoly * N)), dim3(256), 0, st, f, a, min_sz(a.len, out_len), b, min_sz(b.len, out_len),
                           N, 2 * npoly * N);
        ntt_on_stream(pc, g, f, N, 2 * npoly, 0);
        hipLaunchKernelGGL(k_poly_pointwise<false>, dim3(blocks(npoly * N)), dim3(256), 0, st, f, (const Fr*)g, N, npoly * N);
        ntt_on_stream(pc, g, f, N, npoly, 1);
        hipLaunchKernelGGL(k_poly_cut, dim3(blocks(npoly * out_len)), dim3(256), 0, st, out, out_len, out_len, out_flip, (const Fr*)g, N,
                           npoly * out_len);
    }
    DEV_TRY(hipGetLastError());
}

// c[poly L + i] = coefficient i of 1 / b_poly, i < L; a zero b_poly[0] raises pc->flag
void enqueue_inverse(PolyCtx* pc, Fr* c, const Operand& b, size_t L, size_t npoly, const InvPlan& pl) {
    hipStream_t st = pc->st;
    if (b.len == 1 && L > 1) DEV_TRY(hipMemsetAsync(c, 0, npoly * L * sizeof(Fr), st));  // a constant: the rest of the series is zero
    hipLaunchKernelGGL(k_poly_inv0, dim3(blocks(npoly, 64)), dim3(64), 0, st, c, L, b, pc->flag.as<int>(), npoly);
    if (pl.D0 > 1) hipLaunchKernelGGL(k_poly_inv_direct, dim3((unsigned)npoly), dim3(64), 0, st, c, L, b, pl.D0);
    Fr *f = pc->f.as<Fr>(), *g = pc->g.as<Fr>();
    for (const InvStep& s : pl.steps) {
        const Operand cur = {c, s.m, L, 0};
        hipLaunchKernelGGL(k_poly_pad, dim3(blocks(2 * npoly * s.N)), dim3(256), 0, st, f, b, s.nb, cur, s.m, s.N, 2 * npoly * s.N);
        ntt_on_stream(pc, g, f, s.N, 2 * npoly, 0);
        hipLaunchKernelGGL(k_poly_pointwise<true>, dim3(blocks(npoly * s.N)), dim3(256), 0, st, f, (const Fr*)g, s.N, npoly * s.N);
        ntt_on_stream(pc, g, f, s.N, npoly, 1);
        hipLaunchKernelGGL(k_poly_cut, dim3(blocks(npoly * s.n1)), dim3(256), 0, st, c, L, s.n1, 0, (const Fr*)g, s.N, npoly * s.n1);
    }
    DEV_TRY(hipGetLastError());
}

}  // namespace

extern "C" void* kzgamd_poly_new(void* vntt, const KzgAmdConfig* cfg, int* err) {
    int dummy;
    if (!err) err = &dummy;
    *err = 0;
    NttCtx* ntt = (NttCtx*)vntt;
    if (!ntt) {
        *err = -1;
        return nullptr;
    }
    kzgamd::Options opt;
    std::string msg;
    if (!kzgamd::Options::resolve(opt, cfg, &msg)) {
        fprintf(stderr, "kzg_mi355x: kzgamd_poly_new: %s\n", msg.c_str());
        *err = -2;
        return nullptr;
    }
    return kzgamd::create_handle<PolyCtx>(ntt->device, err, [&](PolyCtx* pc) {
        pc->ntt = ntt;
        DEV_TRY(hipStreamCreateWithFlags(&pc->st, hipStreamNonBlocking));
        pc->flag.ensure(sizeof(int));
    });
}

extern "C" void kzgamd_poly_free(void* vpc) {
    PolyCtx* pc = (PolyCtx*)vpc;
    if (!pc) return;
    kzgamd::DeviceGuard on_device(pc->device);
    delete pc;
}

extern "C" int kzgamd_poly_info(void* vpc, size_t* max_width, size_t* eval_chunk, size_t* mul_direct_max, size_t* inv_direct_max) {
    PolyCtx* pc = (PolyCtx*)vpc;
    if (!pc) return -1;
    if (max_width) *max_width = pc->ntt->W;
    if (eval_chunk) *eval_chunk = CHUNK;
    if (mul_direct_max) *mul_direct_max = MUL_DIRECT_MAX;
    if (inv_direct_max) *inv_direct_max = INV_DIRECT_MAX;
    return 0;
}

extern "C" size_t kzgamd_poly_transform_len(int op, size_t la, size_t lb, size_t out_len) {
    if (op == 0) return mul_transform_len(la, lb, out_len);
    if (op == 1) return lb && out_len ? inv_plan(lb, out_len).maxN : 0;
    if (op == 2) return div_transform_len(la, lb);
    return 0;
}

extern "C" int kzgamd_poly_eval(void* vpc, blst_fr* ys, const blst_fr* polys, size_t len, size_t npoly, const blst_fr* xs, size_t nx) {
    PolyCtx* pc = (PolyCtx*)vpc;
    if (!pc) return -1;
    if (npoly == 0 || nx == 0) return 0;
    if (!ys || !xs || (len && !polys)) return -1;
    if (len == 0) {
        memset(ys, 0, npoly * nx * sizeof(blst_fr));
        return 0;
    }
    EvalShape s;
    s.len = len;
    s.nx = nx;
    s.M = (len + CHUNK - 1) / CHUNK;
    s.gw = 1;
    while (s.gw < 64 && s.gw < s.M) s.gw <<= 1;
    s.wv = (u32)((s.M + 63) / 64);
    return run_call(pc, [&] {
        const size_t per = slice_of(pc, npoly, (len + nx * (1 + (s.wv > 1 ? s.wv : 0))) * sizeof(Fr));
        pc->xs.ensure(nx * sizeof(Fr));
        pc->pw.ensure(nx * PW * sizeof(Fr));
        pc->a.ensure(per * len * sizeof(Fr));
        pc->out.ensure(per * nx * sizeof(Fr));
        if (s.wv > 1) pc->sums.ensure(per * nx * s.wv * sizeof(Fr));
        hipStream_t st = pc->st;
        upload(pc, pc->xs.p, xs, nx * sizeof(Fr));
        hipLaunchKernelGGL(k_kzg_pows, dim3(blocks(nx, 64)), dim3(64), 0, st, pc->pw.as<Fr>(), pc->xs.as<Fr>(), (size_t)1, nx);
        for (size_t done = 0; done < npoly; done += per) {
            const size_t cnt = min_sz(per, npoly - done);
            upload(pc, pc->a.p, polys + done * len, cnt * len * sizeof(Fr));
            s.nseq = cnt * nx;
            hipLaunchKernelGGL(k_poly_eval, dim3(blocks(s.nseq * s.gw * s.wv)), dim3(256), 0, st, pc->out.as<Fr>(), pc->sums.as<Fr>(),
                               pc->a.as<Fr>(), pc->pw.as<Fr>(), s);
            if (s.wv > 1)
                hipLaunchKernelGGL(k_poly_eval_carry, dim3((unsigned)s.nseq), dim3(64), 0, st, pc->out.as<Fr>(), pc->sums.as<Fr>(),
                                   pc->pw.as<Fr>(), s);
            DEV_TRY(hipGetLastError());
            download(pc, ys + done * nx, pc->out.p, cnt * nx * sizeof(Fr));
        }
    });
}

extern "C" int kzgamd_poly_scale(void* vpc, blst_fr* out, const blst_fr* in, size_t len, size_t npoly, int inverse) {
    PolyCtx* pc = (PolyCtx*)vpc;
    if (!pc) return -1;
    if (len == 0 || npoly == 0) return 0;
    if (!out || !in) return -1;
    Fr f = Fr::zero();
    f.v[0] = 5;  // SCALE_FACTOR (blst/src/consts.rs)
    f = ff::to_mont(f);
    if (!inverse) f = ff::inverse_bgcd(f);
    return run_call(pc, [&] {
        const size_t per = slice_of(pc, npoly, len * sizeof(Fr));
        pc->a.ensure(per * len * sizeof(Fr));
        for (size_t done = 0; done < npoly; done += per) {
            const size_t cnt = min_sz(per, npoly - done);
            upload(pc, pc->a.p, in + done * len, cnt * len * sizeof(Fr));
            hipLaunchKernelGGL(k_poly_scale, dim3(blocks(cnt * len)), dim3(256), 0, pc->st, pc->a.as<Fr>(), pc->a.as<Fr>(), f, len, cnt * len);
            DEV_TRY(hipGetLastError());
            download(pc, out + done * len, pc->a.p, cnt * len * sizeof(Fr));
        }
    });
}

extern "C" int kzgamd_poly_mul(void* vpc, blst_fr* out, const blst_fr* a, size_t la, const blst_fr* b, size_t lb, size_t out_len,
                               size_t npoly, int form) {
    PolyCtx* pc = (PolyCtx*)vpc;
    if (!pc || form < 0 || form > 2) return -1;
    if (out_len == 0 || npoly == 0) return 0;
    if (!out || (la && !a) || (lb && !b)) return -1;
    if (la == 0 || lb == 0) {
        memset(out, 0, npoly * out_len * sizeof(blst_fr));
        return 0;
    }
    const bool direct = mul_is_direct(la, lb, out_len, form);
    const size_t N = direct ? 0 : mul_transform_len(la, lb, out_len);
    if (N > pc->ntt->W) return 4;
    return run_call(pc, [&] {
        const size_t per = slice_of(pc, npoly, (la + lb + out_len + 4 * N) * sizeof(Fr));
        pc->a.ensure(per * la * sizeof(Fr));
        pc->b.ensure(per * lb * sizeof(Fr));
        pc->out.ensure(per * out_len * sizeof(Fr));
        if (N) {
            pc->f.ensure(2 * per * N * sizeof(Fr));
            pc->g.ensure(2 * per * N * sizeof(Fr));
        }
        for (size_t done = 0; done < npoly; done += per) {
            const size_t cnt = min_sz(per, npoly - done);
            upload(pc, pc->a.p, a + done * la, cnt * la * sizeof(Fr));
            upload(pc, pc->b.p, b + done * lb, cnt * lb * sizeof(Fr));
            enqueue_mul(pc, pc->out.as<Fr>(), out_len, 0, Operand{pc->a.as<Fr>(), la, la, 0}, Operand{pc->b.as<Fr>(), lb, lb, 0}, cnt, form);
            download(pc, out + done * out_len, pc->out.p, cnt * out_len * sizeof(Fr));
        }
    });
}

extern "C" int kzgamd_poly_inverse(void* vpc, blst_fr* out, const blst_fr* b, size_t lb, size_t out_len, size_t npoly) {
    PolyCtx* pc = (PolyCtx*)vpc;
    if (!pc) return -1;
    // the reference's checks in the reference's order (poly.rs:87-95)
    if (out_len == 0) return 1;
    if (lb == 0) return 2;
    if (npoly == 0) return 0;
    if (!out || !b) return -1;
    const size_t lcut = min_sz(lb, out_len);  // coefficients of b beyond out_len never matter
    const InvPlan pl = inv_plan(lcut, out_len);
    if (pl.maxN > pc->ntt->W) return 4;
    int flag = 0;
    const int rc = run_call(pc, [&] {
        const size_t per = slice_of(pc, npoly, (lb + out_len + 4 * pl.maxN) * sizeof(Fr));
        pc->b.ensure(per * lb * sizeof(Fr));
        pc->c.ensure(per * out_len * sizeof(Fr));
        if (pl.maxN) {
            pc->f.ensure(2 * per * pl.maxN * sizeof(Fr));
            pc->g.ensure(2 * per * pl.maxN * sizeof(Fr));
        }
        DEV_TRY(hipMemsetAsync(pc->flag.p, 0, sizeof(int), pc->st));
        for (size_t done = 0; done < npoly; done += per) {
            const size_t cnt = min_sz(per, npoly - done);
            upload(pc, pc->b.p, b + done * lb, cnt * lb * sizeof(Fr));
            enqueue_inverse(pc, pc->c.as<Fr>(), Operand{pc->b.as<Fr>(), lcut, lb, 0}, out_len, cnt, pl);
            download(pc, out + done * out_len, pc->c.p, cnt * out_len * sizeof(Fr));
        }
        download(pc, &flag, pc->flag.p, sizeof(int));
    });
    return rc ? rc : (flag ? 3 : 0);
}

extern "C" int kzgamd_poly_div(void* vpc, blst_fr* q, const blst_fr* a, size_t la, const blst_fr* b, size_t lb, size_t npoly) {
    PolyCtx* pc = (PolyCtx*)vpc;
    if (!pc) return -1;
    if (lb == 0) return 1;
    if (npoly == 0 || la < lb) return 0;
    if (!q || !a || !b) return -1;
    const size_t L = la - lb + 1;
    const InvPlan pl = inv_plan(min_sz(lb, L), L);
    const size_t N = div_transform_len(la, lb);
    if (N > pc->ntt->W) return 4;
    int flag = 0;
    const int rc = run_call(pc, [&] {
        const size_t per = slice_of(pc, npoly, (la + lb + 2 * L + 4 * N) * sizeof(Fr));
        pc->a.ensure(per * la * sizeof(Fr));
        pc->b.ensure(per * lb * sizeof(Fr));
        pc->c.ensure(per * L * sizeof(Fr));
        pc->out.ensure(per * L * sizeof(Fr));
        if (N) {
            pc->f.ensure(2 * per * N * sizeof(Fr));
            pc->g.ensure(2 * per * N * sizeof(Fr));
        }
        hipStream_t st = pc->st;
        DEV_TRY(hipMemsetAsync(pc->flag.p, 0, sizeof(int), st));
        for (size_t done = 0; done < npoly; done += per) {
            const size_t cnt = min_sz(per, npoly - done);
            upload(pc, pc->a.p, a + done * la, cnt * la * sizeof(Fr));
            upload(pc, pc->b.p, b + done * lb, cnt * lb * sizeof(Fr));
            if (lb == 1) {
                // a constant divisor (poly.rs:231-240): one inversion per polynomial, a product per coefficient
                hipLaunchKernelGGL(k_poly_inv0, dim3(blocks(cnt, 64)), dim3(64), 0, st, pc->c.as<Fr>(), (size_t)1,
                                   Operand{pc->b.as<Fr>(), 1, 1, 0}, pc->flag.as<int>(), cnt);
                hipLaunchKernelGGL(k_poly_mul_const, dim3(blocks(cnt * la)), dim3(256), 0, st, pc->out.as<Fr>(), pc->a.as<Fr>(),
                                   pc->c.as<Fr>(), la, cnt * la);
                DEV_TRY(hipGetLastError());
            } else {
                // fast_div (poly.rs:242-249): q = flip(flip(a) * (1 / flip(b) mod x^L) mod x^L)
                enqueue_inverse(pc, pc->c.as<Fr>(), Operand{pc->b.as<Fr>(), lb, lb, 1}, L, cnt, pl);
                enqueue_mul(pc, pc->out.as<Fr>(), L, 1, Operand{pc->a.as<Fr>(), la, la, 1}, Operand{pc->c.as<Fr>(), L, L, 0}, cnt, 0);
            }
            download(pc, q + done * L, pc->out.p, cnt * L * sizeof(Fr));
        }
        download(pc, &flag, pc->flag.p, sizeof(int));
    });
    return rc ? rc : (flag ? 2 : 0);
}
