// Generic polynomial KZG: the proving and checking calls of the reference's KZGSettings
// (blst/src/types/kzg_settings.rs:138-277: commit_to_poly, compute_proof_single, compute_proof_multi, check_proof_single,
// check_proof_multi) for any setup [s^i]G, batched: npoly polynomials x nx points per open call, count tuples per check.
//
// A proof is the commitment to the quotient q of p = q (X^n - c) + r, c = x^n, deg r < n.  With h_j = p_j + c h_{j+n}
// (h_j = 0 for j >= len) the quotient is q_j = h_{j+n} and the remainder r_j = h_j, j < n: n independent first-order
// recurrences with the SAME multiplier c — one per residue rho = j mod n, the sequence a_t = p_{rho + t n}, t < T =
// ceil(len / n), run from the top.  Two kernel forms, taken by shape (kzgamd_kzg_info gives the threshold):
//   lane form     one lane per (pair, rho), serial over t; neighbouring lanes hold neighbouring rho, so every step is a
//                 coalesced 32-byte-per-lane load and store.  Taken when the call has LANE_FORM_MIN such lanes or more.
//   chunked scan  one lane per (pair, rho, chunk m of CHUNK consecutive t).  The lane runs its chunk from a zero carry: S_m.
//                 The true value at the base of chunk m is H_m = S_m + C H_{m+1}, C = c^CHUNK — the same recurrence one
//                 level up — solved inside a wave by a log-step suffix scan over lanes with the powers C^(2^k), k < 6,
//                 and across waves through one summary per wave in global memory: k_kzg_chunk<false> writes the S_m
//                 and the summaries, k_kzg_carry turns the summaries into the true values at the wave bases (the same
//                 scan once more, a lane per wave, with the powers of C^64), k_kzg_chunk<true> scans the S_m again from
//                 them and replays every chunk from its true incoming carry, writing q and r.  A sequence of up to 64
//                 chunks takes the last launch alone, in a group of 1, 2, .. 64 lanes of a wave.
//                 A dependent multiplication is ~1.1 us on a wave that has its SIMD to itself (measured, profiles/NOTES.md):
//                 the depth of the three launches — CHUNK + 6, 6 and 6 + CHUNK multiplications — is what they cost.
// Both write q pair-major in Montgomery form, what msm_enqueue(mont = 1) reads, and r for the evaluations: ys = forward
// transform of r_j x^j.  Wave-local exchange and global memory between launches only: no workgroup barrier in this file.
// Everything between the upload of the coefficients and the download of the proofs is enqueued on the handle's one
// stream; a call holds the handle's lock and synchronises before it returns.
//
// check: the G1 side com - [I(s)]G for all tuples on the GPU (inverse transform of the ys, x^-i by one inversion per
// tuple, one MSM per tuple over the first n setup points, the subtraction); the G2 side and one pairing per tuple on
// the host (host_pairing.h), as in the reference.
//
// check_batch: any number of tuples under ONE pairing.  With weights rho_t = r^t,
//     L = sum rho_t C_t + sum rho_t x_t^n pi_t - [A(s)]G,  A = sum rho_t I_t,   P = sum rho_t pi_t,   ok = e(L, G2) == e(P, [s^n]G2).
// GPU: the 2 count Jacobian points to affine slots with the curve equation tested (k_kzg_points: Montgomery's trick, one
// inversion per lane) and the r-torsion test on each (k_kzg_in_g1), failures counted in two status words the host reads
// once; the weights and the two scalar rows over [proofs | commitments] (k_kzg_batch_scalars); A from one batched inverse
// transform (k_kzg_batch_agg: a lane per tuple walks x^-i, wave shuffles sum over the tuples; k_kzg_batch_fold adds the
// waves); [A(s)]G on the setup's MSM handle, one two-row variable-base MSM over the checked points, one
// subtraction, one download.  Host: the SHA-256 of the challenge before the handle's lock is taken (a hash of megabytes
// at large counts must not hold up the handle's other callers), one pairing check after it is released, against the line
// tables of G2 (pairing::prepared_lines) and of [s^n]G2, kept per handle and n.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kzg_mi355x.h"
#include "config.h"
#include "device_guard.h"
#include "ff.hip.h"
#include "fr29.hip.h"
#include "frscan.hip.h"
#include "g1_28.hip.h"
#include "g1_io.hip.h"
#include "host_call.h"
#include "host_fp64.h"
#include "host_g1.h"
#include "host_pairing.h"
#include "msm_internal.h"
#include "glv.hip.h"
#include "ntt_internal.h"
#include "pairing_internal.h"
#include "sha256.h"

using ff::Fr;
using ff::u32;
using g1::AffPt;
using g1::Xyzz;
using kzgamd::blocks;
using kzgamd::DevBuf;
using kzgamd::DevErr;

namespace {

// CHUNK, PW, NPOW, fr_mul, fr_pow, shfl_down, scan_suffix and k_kzg_pows: frscan.hip.h, shared with poly.hip
constexpr size_t LANE_FORM_MIN = 16384;     // lanes (pairs x n) from which the lane form is taken: a wave per CU

struct QuotShape {
    size_t len, n, nx, L;    // L = len - n: the quotient's length (the MSMs' stride); only called with len > n
    size_t pair0, npairs;    // the pairs of this pass: pair = poly * nx + x index
    size_t M;                // chunks per sequence, ceil(ceil(len / n) / CHUNK)
    u32 gw, wv;              // lanes of a wave per sequence (a power of two <= 64), waves per sequence (gw == 64 if > 1)
};

// the lane form: thread = (pair, rho)
__global__ void __launch_bounds__(256) k_kzg_lanes(Fr* __restrict__ q, Fr* __restrict__ r, const Fr* __restrict__ polys,
                                                   const Fr* __restrict__ pw, QuotShape s) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= s.npairs * s.n) return;
    const size_t rho = t % s.n, pl = t / s.n, pair = s.pair0 + pl;
    const Fr* p = polys + (pair / s.nx) * s.len;
    const Fr c = pw[(pair % s.nx) * PW];
    Fr* qo = q + pl * s.L;
    Fr acc = Fr::zero();
    if (rho < s.len) {
        for (size_t j = rho + (s.len - 1 - rho) / s.n * s.n;; j -= s.n) {
            acc = ff::add(p[j], fr_mul(c, acc));
            if (j < s.n) break;
            qo[j - s.n] = acc;
        }
    }
    r[pl * s.n + rho] = acc;
}

// the chunked form: thread = (sequence = (pair, rho), chunk m), gw * wv slots per sequence.
// REPLAY == false (wv > 1 only): S_m to local[thread], the summary of the wave, sum_d C^d S_{64 w + d}, to sums[seq * wv + w].
// REPLAY == true: sums holds the true values at the wave bases (k_kzg_carry) and local the S_m when wv > 1 (a sequence
// within one wave computes them here); q and r are written.
template <bool REPLAY>
__global__ void __launch_bounds__(256) k_kzg_chunk(Fr* __restrict__ q, Fr* __restrict__ r, Fr* __restrict__ sums, Fr* __restrict__ local,
                                                   const Fr* __restrict__ polys, const Fr* __restrict__ pw, QuotShape s) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t slots = (size_t)s.gw * s.wv;
    const size_t seq = t / slots, m = t % slots;
    const bool live = seq < s.npairs * s.n && m < s.M;  // dead lanes carry zeros through the scan: no lane leaves early
    const size_t rho = live ? seq % s.n : 0, pl = live ? seq / s.n : 0, pair = s.pair0 + pl;
    const Fr* p = polys + (pair / s.nx) * s.len;
    const Fr* mypw = pw + (pair % s.nx) * PW;
    const Fr c = mypw[0];
    const size_t t0 = m * CHUNK;
    // the chunk from a zero carry
    Fr S = Fr::zero();
    if (REPLAY && s.wv > 1) {
        S = local[t];
    } else if (live) {
        for (int i = CHUNK - 1; i >= 0; --i) {
            const size_t j = rho + (t0 + i) * s.n;
            if (j < s.len) S = ff::add(p[j], fr_mul(c, S));
        }
    }
    if (!REPLAY) local[t] = S;
    const u32 lg = (u32)(m & (s.gw - 1));        // lane within the group
    const size_t w = m / 64;                      // wave within the sequence (0 when gw < 64)
    const bool more = REPLAY && live && s.wv > 1 && w + 1 < s.wv;  // a wave of this sequence above this one
    Fr above = Fr::zero();                        // true value at the base of the next wave
    if (more) above = sums[seq * s.wv + w + 1];
    if (more && lg == 63) S = ff::add(S, fr_mul(mypw[1], above));
    // suffix scan over the group: H_m = sum_{d >= 0} C^d S_{m + d}
    const Fr H = scan_suffix(S, lg, s.gw, mypw + 1);
    if (!REPLAY) {
        if (live && lg == 0) sums[seq * s.wv + w] = H;
        return;
    }
    Fr acc = shfl_down(H, 1);                     // H_{m+1}: the carry into this chunk
    if (lg + 1 >= s.gw) acc = above;
    if (!live) return;
    // the chunk again, from its true carry
    Fr* qo = q + pl * s.L;
    for (int i = CHUNK - 1; i >= 0; --i) {
        const size_t j = rho + (t0 + i) * s.n;
        if (j >= s.len) continue;
        acc = ff::add(p[j], fr_mul(c, acc));
        if (j >= s.n) qo[j - s.n] = acc;
        else r[pl * s.n + rho] = acc;
    }
}

// summaries of the waves of a sequence -> true values at the wave bases, G_w = W_w + C^64 G_{w+1}: a wave per sequence,
// a lane per summary, blocks of 64 summaries from the top, each by the suffix scan of k_kzg_chunk with the powers of C^64
__global__ void __launch_bounds__(64) k_kzg_carry(Fr* __restrict__ sums, const Fr* __restrict__ pw, QuotShape s) {
    const size_t seq = blockIdx.x;  // < npairs * n
    const u32 lane = threadIdx.x;
    const Fr* mypw = pw + ((s.pair0 + seq / s.n) % s.nx) * PW + 7;  // (C^64)^(2^k), k = 0 .. 5
    Fr* g = sums + seq * s.wv;
    Fr above = Fr::zero();
    for (size_t blk = (s.wv + 63) / 64; blk-- > 0;) {
        const size_t w = blk * 64 + lane;
        Fr H = w < s.wv ? g[w] : Fr::zero();
        if (lane == 63) H = ff::add(H, fr_mul(mypw[0], above));
        H = scan_suffix(H, lane, 64, mypw);
        if (w < s.wv) g[w] = H;
#pragma unroll
        for (int i = 0; i < 8; ++i) above.v[i] = __shfl(H.v[i], 0, 64);
    }
}

// r_j *= x^j, j < n, for every pair: the forward transform of the result is p(x w^i)
__global__ void __launch_bounds__(256) k_kzg_twist(Fr* __restrict__ r, const Fr* __restrict__ xs, size_t n, size_t nx, size_t pair0,
                                                   size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t j = t % n;
    if (j == 0) return;
    r[t] = fr_mul(r[t], fr_pow(xs[(pair0 + t / n) % nx], j));
}
// xs[t] = 1 / xs[t]
__global__ void __launch_bounds__(64) k_kzg_invert(Fr* __restrict__ xs, size_t count) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count) xs[t] = ff::inverse_bgcd(xs[t]);
}
// interp[tuple][i] *= (1 / x_tuple)^i
__global__ void __launch_bounds__(256) k_kzg_unscale(Fr* __restrict__ v, const Fr* __restrict__ xinv, size_t n, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t i = t % n;
    if (i == 0) return;
    v[t] = fr_mul(v[t], fr_pow(xinv[t / n], i));
}
// out = a - b, blst Jacobian points
__global__ void __launch_bounds__(64) k_kzg_g1_sub(ff::Fp* __restrict__ out, const ff::Fp* __restrict__ a, const ff::Fp* __restrict__ b,
                                                   size_t count) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    auto load = [](const ff::Fp* src) {
        Xyzz p;
        if (src[2].is_zero()) {
            g1::set_inf(p);
        } else {
            const fp28::Fe z = fp28::from_blst(src[2]);
            p.x = fp28::from_blst(src[0]);
            p.y = fp28::from_blst(src[1]);
            p.zz = fp28::sqr(z);
            p.zzz = fp28::mul(p.zz, z);
        }
        return p;
    };
    Xyzz A = load(a + 3 * t), B = load(b + 3 * t);
    if (!g1::is_inf(B)) B.y = fp28::neg<8>(B.y);
    g1::dadd(A, B);
    g1::to_blst_jacobian(out + 3 * t, A);
}

// ---- check on the GPU (pairing.hip) ----
// flags[t] = 1 when slot t is in the r-torsion subgroup (what k_kzg_in_g1 counts per call, kept per point): a tuple
// whose commitment or proof is outside G1 goes to the host loop, because the GLV multiplication and the rearrangement
// e(lhs + [x^n] proof, G2) == e(proof, [s^n]G2) only hold in G1
__global__ void __launch_bounds__(64) k_kzg_in_g1_each(const AffPt* __restrict__ pts, size_t total, uint8_t* __restrict__ flags) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    flags[t] = g1io::affpt_in_g1(pts[t]) ? 1 : 0;
}
// out = a + b: a blst Jacobian, b g1::Xyzz (the products [x^n] proof), out blst Jacobian
__global__ void __launch_bounds__(64) k_kzg_g1_add_xyzz(ff::Fp* __restrict__ out, const ff::Fp* __restrict__ a, const Xyzz* __restrict__ b,
                                                        size_t count) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const ff::Fp* src = a + 3 * t;
    Xyzz A;
    if (src[2].is_zero()) {
        g1::set_inf(A);
    } else {
        const fp28::Fe z = fp28::from_blst(src[2]);
        A.x = fp28::from_blst(src[0]);
        A.y = fp28::from_blst(src[1]);
        A.zz = fp28::sqr(z);
        A.zzz = fp28::mul(A.zz, z);
    }
    g1::dadd(A, b[t]);
    g1::to_blst_jacobian(out + 3 * t, A);
}

// ---- check_batch ----
constexpr int PT_CHUNK = 8;        // points per lane of k_kzg_points: one inversion per PT_CHUNK points
constexpr int AGG_WAVE = 64;       // tuples per block of k_kzg_batch_agg: one wave

// blst Jacobian points -> the affine slots of the variable-base engine (identity: flag and (0, 0)), a lane per PT_CHUNK
// consecutive points with one inversion of the product of their Z (pref: a slot per point for the running products).
// The curve equation is tested on what the lane has just computed, y^2 == x^3 + 4 with x = X / Z^2, y = Y / Z^3 — which
// is Y^2 == X^3 + 4 Z^6 for Z != 0; a point that fails becomes the identity and counts in status[0].
// The identity is Z with all-zero limbs, whatever X and Y hold (blst's convention).  Coordinates are taken mod p: a
// non-canonical one (>= p) is the element it reduces to.  The one exception fails safe: a Z that is 0 mod p with non-zero
// limbs (Z = p) zeroes the lane's running product, the inverse of 0 comes back 0, and all PT_CHUNK points of the lane fail
// the curve test — the call returns 7, as it would for that point alone.
__global__ void __launch_bounds__(64) k_kzg_points(AffPt* __restrict__ out, const ff::Fp* __restrict__ jac, fp28::Fe* __restrict__ pref,
                                                   size_t total, int* __restrict__ status) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t lo = t * PT_CHUNK;
    if (lo >= total) return;
    const size_t hi = lo + PT_CHUNK < total ? lo + PT_CHUNK : total;
    fp28::Fe run = fp28::one();
    for (size_t k = lo; k < hi; ++k) {
        pref[k] = run;
        if (!jac[3 * k + 2].is_zero()) run = fp28::mul(run, fp28::from_blst(jac[3 * k + 2]));
    }
    fp28::Fe inv = g1io::inverse(run);
    fp28::Fe b4;
#pragma unroll
    for (int i = 0; i < 14; ++i) b4.v[i] = g1io::b4_392_l(i);
    int bad = 0;
    for (size_t k = hi; k-- > lo;) {
        AffPt o;
        o.flags = 1;
        o.pad[0] = o.pad[1] = o.pad[2] = 0;
        o.x = fp28::zero();
        o.y = fp28::zero();
        if (!jac[3 * k + 2].is_zero()) {
            const fp28::Fe z = fp28::from_blst(jac[3 * k + 2]);
            const fp28::Fe zi = fp28::mul(inv, pref[k]), zi2 = fp28::sqr(zi);
            inv = fp28::mul(inv, z);
            const fp28::Fe x = fp28::mul(fp28::from_blst(jac[3 * k]), zi2);
            const fp28::Fe y = fp28::mul(fp28::from_blst(jac[3 * k + 1]), fp28::mul(zi2, zi));
            const fp28::Fe rhs = fp28::addn(fp28::mul(fp28::sqr(x), x), b4);  // x^3 + 4, < 4p
            if (fp28::is_zero_mod_p(fp28::sub<8>(fp28::sqr(y), rhs))) {
                o.flags = 0;
                o.x = fp28::canon(x);
                o.y = fp28::canon(y);
            } else {
                ++bad;
            }
        }
        out[k] = o;
    }
    if (bad) atomicAdd(status, bad);
}
// the r-torsion test of every slot (g1_io.hip.h: phi(P) == -[x^2]P, what k_bases_in_g1 runs on a handle's bases): status[1]
__global__ void __launch_bounds__(64) k_kzg_in_g1(const AffPt* __restrict__ pts, size_t total, int* __restrict__ status) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    if (!g1io::affpt_in_g1(pts[t])) atomicAdd(status + 1, 1);
}
// per tuple: rho_t = r^t, and the two scalar rows over [proofs | commitments] (np = 2 count columns):
// row P = rho_t | 0, row L = rho_t x_t^n | rho_t
__global__ void __launch_bounds__(64) k_kzg_batch_scalars(Fr* __restrict__ rho, Fr* __restrict__ rows, const Fr* __restrict__ r,
                                                          const Fr* __restrict__ xs, size_t n, size_t count) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const Fr w = fr_pow(*r, t);
    Fr xn = xs[t];
    for (size_t m = 1; m < n; m <<= 1) xn = fr_mul(xn, xn);
    rho[t] = w;
    rows[t] = w;
    rows[count + t] = Fr::zero();
    rows[2 * count + t] = fr_mul(w, xn);
    rows[3 * count + t] = w;
}
// part[wave][i] = sum over the 64 tuples t of the wave of rho_t x_t^-i v_t[i], i < n: a lane per tuple walks rho_t x_t^-i
// along i, the sum over t by shuffles; a block is one wave, so nothing here needs a workgroup barrier (k_kzg_batch_fold
// adds the waves).  xinv == nullptr (n = 1): no walk.  Field addition is exact: the order of the sum does not matter.
__global__ void __launch_bounds__(AGG_WAVE) k_kzg_batch_agg(Fr* __restrict__ part, const Fr* __restrict__ v, const Fr* __restrict__ rho,
                                                            const Fr* __restrict__ xinv, size_t n, size_t count) {
    const size_t t = (size_t)blockIdx.x * AGG_WAVE + threadIdx.x;
    const bool live = t < count;  // dead lanes add zeros: no lane leaves before the shuffles
    Fr pw = live ? rho[t] : Fr::zero();
    const Fr step = live && xinv ? xinv[t] : Fr::zero();
    const Fr* mine = v + (live ? t : 0) * n;
    Fr* out = part + (size_t)blockIdx.x * n;
    for (size_t i = 0; i < n; ++i) {
        Fr term = live ? fr_mul(pw, mine[i]) : Fr::zero();
        if (i + 1 < n) pw = fr_mul(pw, step);
        for (int d = 32; d > 0; d >>= 1) term = ff::add(term, shfl_down(term, d));
        if (threadIdx.x == 0) out[i] = term;
    }
}
// A_i = sum over the waves of part[wave][i]
__global__ void __launch_bounds__(256) k_kzg_batch_fold(Fr* __restrict__ agg, const Fr* __restrict__ part, size_t n, size_t nblocks) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr s = part[i];
    for (size_t b = 1; b < nblocks; ++b) s = ff::add(s, part[b * n + i]);
    agg[i] = s;
}

// Built-in pairing_gpu_min (tuning key of kzgamd_kzg_new; -1 selects this): the smallest count at which the GPU form of check_each beat the
// host loop in tools/time_pairing_batch.py (profiles/pairing_batch_time.jsonl, NOTES 33)
constexpr size_t PAIRING_GPU_MIN_DEFAULT = 4;

struct KzgCtx {
    NttCtx* ntt = nullptr;
    int device = 0;
    size_t num_g1 = 0, num_g2 = 0;
    std::vector<kzgamd::pairing::G2Jac> g2;
    std::mutex mu;
    hipStream_t st = nullptr;
    kzgamd::MsmContext* msm = nullptr;
    // check_batch: the variable-base handle over a call's checked points (created by the first call, given new points by
    // every later one), and the line table of [s^n]G2 per n (G2's own comes from pairing::prepared_lines)
    kzgamd::Options opt;
    kzgamd::MsmContext* vmsm = nullptr;
    std::map<size_t, std::shared_ptr<const kzgamd::pairing::LineTable>> lines;
    // check on the GPU: the count from which check_each takes it (0 = never), the device line tables of G2 and of
    // [s^n]G2 per n, kept for the life of the handle
    size_t pairing_gpu_min = 0;
    kzgamd::pairing_gpu::DeviceTable dgen;
    bool have_dgen = false;
    std::map<size_t, kzgamd::pairing_gpu::DeviceTable> dlines;
    // workspace, grown as calls need it
    DevBuf polys, xs, pw, q, r, r2, sums, local, out, pts;
    DevBuf aff, pref, stat, xinv, rho, rows, part, agg;
    DevBuf gjac, gflags, gsplit, gxyzz, gprod, gtab, gsum, gok;

    ~KzgCtx() {
        if (vmsm) kzgamd::msm_destroy(vmsm);
        if (msm) kzgamd::msm_destroy(msm);
        if (st) (void)hipStreamDestroy(st);
    }
};

// nbatch MSMs of npoints scalars (Montgomery, stride npoints) over the first setup points, Jacobian out, on the stream
void msm_on_stream(KzgCtx* kz, void* d_out, const void* d_scalars, size_t npoints, size_t nbatch) {
    kzgamd::MsmLock locked(kz->msm);
    kzgamd::msm_enqueue(kz->msm, d_out, d_scalars, npoints, nbatch, 1, kz->st, kzgamd::OUT_JACOBIAN);
}

// the quotients and remainders of the pairs [pair0, pair0 + npairs) into kz->q (stride len - n) and kz->r (stride n)
void enqueue_quotients(KzgCtx* kz, size_t len, size_t n, size_t nx, size_t pair0, size_t npairs) {
    QuotShape s;
    s.len = len;
    s.n = n;
    s.nx = nx;
    s.L = len - n;
    s.pair0 = pair0;
    s.npairs = npairs;
    const size_t T = (len + n - 1) / n, seqs = npairs * n;
    s.M = (T + CHUNK - 1) / CHUNK;
    s.gw = 1;
    while (s.gw < 64 && s.gw < s.M) s.gw <<= 1;
    s.wv = (u32)((s.M + 63) / 64);
    Fr *q = kz->q.as<Fr>(), *r = kz->r.as<Fr>();
    const Fr *p = kz->polys.as<Fr>(), *pw = kz->pw.as<Fr>();
    if (seqs >= LANE_FORM_MIN) {
        hipLaunchKernelGGL(k_kzg_lanes, dim3(blocks(seqs)), dim3(256), 0, kz->st, q, r, p, pw, s);
    } else {
        const size_t threads = seqs * s.gw * s.wv;
        Fr *sums = nullptr, *local = nullptr;
        if (s.wv > 1) {
            kz->sums.ensure(seqs * s.wv * sizeof(Fr));
            kz->local.ensure((size_t)blocks(threads) * 256 * sizeof(Fr));
            sums = kz->sums.as<Fr>();
            local = kz->local.as<Fr>();
            hipLaunchKernelGGL(k_kzg_chunk<false>, dim3(blocks(threads)), dim3(256), 0, kz->st, q, r, sums, local, p, pw, s);
            hipLaunchKernelGGL(k_kzg_carry, dim3((unsigned)seqs), dim3(64), 0, kz->st, sums, pw, s);
        }
        hipLaunchKernelGGL(k_kzg_chunk<true>, dim3(blocks(threads)), dim3(256), 0, kz->st, q, r, sums, local, p, pw, s);
    }
    DEV_TRY(hipGetLastError());
}

}  // namespace

extern "C" void* kzgamd_kzg_new(void* vntt, const blst_p1* g1_monomial, size_t num_g1, const blst_p2* g2_monomial, size_t num_g2,
                                const KzgAmdConfig* cfg, int* err) {
    int dummy;
    if (!err) err = &dummy;
    *err = 0;
    NttCtx* ntt = (NttCtx*)vntt;
    if (num_g1 == 0) {
        *err = 1;
        return nullptr;
    }
    if (!ntt || !g1_monomial || (num_g2 && !g2_monomial)) {
        *err = -1;
        return nullptr;
    }
    // pairing_gpu_min is a key of this handle type alone (as fk20_table is of kzgamd_fk20_new): it is taken out of
    // cfg->tuning here, the rest goes to the library's table of keys (config.h) as for every other handle
    long long gpu_min = -1;
    KzgAmdConfig local;
    std::string rest, msg;
    if (cfg && cfg->struct_size >= offsetof(KzgAmdConfig, tuning) + sizeof(cfg->tuning) && cfg->tuning) {
        if (!kzgamd::take_key(cfg->tuning, "pairing_gpu_min", -1, 1 << 20, &gpu_min, &rest)) {
            fprintf(stderr, "kzg_mi355x: kzgamd_kzg_new: tuning: 'pairing_gpu_min' takes -1 ... 1048576\n");
            *err = -2;
            return nullptr;
        }
        local = *cfg;
        local.tuning = rest.c_str();
        cfg = &local;
    }
    kzgamd::Options opt;
    if (!kzgamd::Options::resolve(opt, cfg, &msg)) {
        fprintf(stderr, "kzg_mi355x: kzgamd_kzg_new: %s\n", msg.c_str());
        *err = -2;
        return nullptr;
    }
    opt.device = ntt->device;  // the handle lives where its NTT handle lives
    return kzgamd::create_handle<KzgCtx>(ntt->device, err, [&](KzgCtx* kz) {
        kz->ntt = ntt;
        kz->opt = opt;
        kz->pairing_gpu_min = gpu_min < 0 ? PAIRING_GPU_MIN_DEFAULT : (size_t)gpu_min;
        kz->num_g1 = num_g1;
        kz->num_g2 = g2_monomial ? num_g2 : 0;
        kz->g2.resize(kz->num_g2);
        if (kz->num_g2) memcpy(kz->g2.data(), g2_monomial, kz->num_g2 * sizeof(blst_p2));
        DEV_TRY(hipStreamCreateWithFlags(&kz->st, hipStreamNonBlocking));
        std::vector<ff::Fp> aff(2 * num_g1);  // the setup points as blst affine points
        kzgamd::host_p1_to_affine_batch(aff.data(), num_g1, [&](size_t i) { return &g1_monomial[i]; });
        kz->msm = kzgamd::msm_create(aff.data(), num_g1, false, true, false, kzgamd::G1_CHECK, &opt);
    });
}

extern "C" void kzgamd_kzg_free(void* vkz) {
    KzgCtx* kz = (KzgCtx*)vkz;
    if (!kz) return;
    kzgamd::DeviceGuard on_device(kz->device);
    delete kz;
}

extern "C" int kzgamd_kzg_info(void* vkz, size_t* num_g1, size_t* num_g2, size_t* chunk, size_t* lane_form_min) {
    KzgCtx* kz = (KzgCtx*)vkz;
    if (!kz) return -1;
    if (num_g1) *num_g1 = kz->num_g1;
    if (num_g2) *num_g2 = kz->num_g2;
    if (chunk) *chunk = CHUNK;
    if (lane_form_min) *lane_form_min = LANE_FORM_MIN;
    return 0;
}

extern "C" int kzgamd_kzg_commit(void* vkz, blst_p1* out, const blst_fr* polys, size_t len, size_t npoly) {
    KzgCtx* kz = (KzgCtx*)vkz;
    if (!kz) return -1;
    if (len > kz->num_g1) return 1;
    if (npoly == 0) return 0;
    if (!out || (len && !polys)) return -1;
    if (len == 0) {
        memset(out, 0, npoly * sizeof(blst_p1));
        return 0;
    }
    return kzgamd::run_call(kz, [&] {
        kz->polys.ensure(npoly * len * sizeof(Fr));
        kz->out.ensure(npoly * sizeof(blst_p1));
        DEV_TRY(hipMemcpyAsync(kz->polys.p, polys, npoly * len * sizeof(Fr), hipMemcpyHostToDevice, kz->st));
        msm_on_stream(kz, kz->out.p, kz->polys.p, len, npoly);
        DEV_TRY(hipMemcpyAsync(out, kz->out.p, npoly * sizeof(blst_p1), hipMemcpyDeviceToHost, kz->st));
    });
}

extern "C" int kzgamd_kzg_open(void* vkz, blst_p1* proofs, blst_fr* ys, const blst_fr* polys, size_t len, size_t npoly,
                               const blst_fr* xs, size_t nx, size_t n) {
    KzgCtx* kz = (KzgCtx*)vkz;
    if (!kz) return -1;
    // the reference's checks in the reference's order (kzg_settings.rs:155-158, 198-205, 138-141)
    if (len == 0) return 2;
    if (n == 0 || (n & (n - 1))) return 3;
    if (len > n && len - n > kz->num_g1) return 1;
    if (ys && n > kz->ntt->W) return 4;
    const size_t npairs = npoly * nx;
    if (npairs == 0) return 0;
    if (!proofs || !polys || !xs) return -1;
    return kzgamd::run_call(kz, [&] {
        // the workspace of a pass (quotients, remainders, the MSM's digits beside them) stays within a share of the free
        // HBM: a larger call runs in slices of pairs
        size_t free_b = 0, total_b = 0;
        DEV_TRY(hipMemGetInfo(&free_b, &total_b));
        const size_t per_pair = (len + 2 * n) * sizeof(Fr) + sizeof(blst_p1);
        size_t per = (free_b + kz->q.cap + kz->r.cap + kz->r2.cap) / 8 / per_pair;
        if (per == 0) per = 1;
        if (per > npairs) per = npairs;
        const size_t L = len > n ? len - n : 0;
        kz->polys.ensure(npoly * len * sizeof(Fr));
        kz->xs.ensure(nx * sizeof(Fr));
        kz->pw.ensure(nx * PW * sizeof(Fr));
        kz->q.ensure(per * L * sizeof(Fr));
        kz->r.ensure(per * n * sizeof(Fr));
        if (ys && n > 1) kz->r2.ensure(per * n * sizeof(Fr));
        kz->out.ensure(per * sizeof(blst_p1));
        hipStream_t st = kz->st;
        DEV_TRY(hipMemcpyAsync(kz->polys.p, polys, npoly * len * sizeof(Fr), hipMemcpyHostToDevice, st));
        DEV_TRY(hipMemcpyAsync(kz->xs.p, xs, nx * sizeof(Fr), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_kzg_pows, dim3(blocks(nx, 64)), dim3(64), 0, st, kz->pw.as<Fr>(), kz->xs.as<Fr>(), n, nx);
        for (size_t done = 0; done < npairs; done += per) {
            const size_t cnt = npairs - done < per ? npairs - done : per;
            if (L == 0) {
                // len <= n: the reference's zero-length quotient (poly.rs:167-170, 226-229); r = p, zero-extended
                DEV_TRY(hipMemsetAsync(kz->out.p, 0, cnt * sizeof(blst_p1), st));
                if (ys) {
                    DEV_TRY(hipMemsetAsync(kz->r.p, 0, cnt * n * sizeof(Fr), st));
                    for (size_t i = 0; i < cnt; ++i)
                        DEV_TRY(hipMemcpyAsync(kz->r.as<Fr>() + i * n, kz->polys.as<Fr>() + (done + i) / nx * len, len * sizeof(Fr),
                                              hipMemcpyDeviceToDevice, st));
                }
            } else {
                enqueue_quotients(kz, len, n, nx, done, cnt);
                msm_on_stream(kz, kz->out.p, kz->q.p, L, cnt);
            }
            DEV_TRY(hipMemcpyAsync(proofs + done, kz->out.p, cnt * sizeof(blst_p1), hipMemcpyDeviceToHost, st));
            if (!ys) continue;
            const Fr* vals = kz->r.as<Fr>();
            if (n > 1) {
                hipLaunchKernelGGL(k_kzg_twist, dim3(blocks(cnt * n)), dim3(256), 0, st, kz->r.as<Fr>(), kz->xs.as<Fr>(), n, nx,
                                   done, cnt * n);
                if (kzgamd_ntt_fr_device(kz->ntt, kz->r2.p, kz->r.p, n, cnt, 0, st) != 0) throw DevErr{hipErrorUnknown};
                vals = kz->r2.as<Fr>();
            }
            DEV_TRY(hipGetLastError());
            DEV_TRY(hipMemcpyAsync(ys + done * n, vals, cnt * n * sizeof(Fr), hipMemcpyDeviceToHost, st));
        }
    });
}

namespace {

// The pairings of check_each on the GPU, for the tuples whose commitment and proof are in G1 (the handle's lock held, the
// stream holding lhs = commitment - [interp(s)]G in `dif`):   e(lhs + [x^n] proof, G2) == e(proof, [s^n]G2),
// the per-tuple G2 term moved to the G1 side as check_batch does.  [x^n] proof by the GLV lanes of g1_varmul_sum_device
// (group = 1), the sums by k_kzg_g1_add_xyzz, the verdicts by one wave per tuple (pairing_internal.h) against the device
// tables of G2 and g2[n].  to_host[t] = 1: the tuple stays with the host loop (a point outside G1, or the identity).
// false: a point off the curve somewhere in the call — every tuple stays with the host loop.  Synchronises the stream.
bool check_each_gpu(KzgCtx* kz, std::vector<uint8_t>& verdict, std::vector<uint8_t>& to_host, const ff::Fp* dif, const blst_p1* proofs,
                    const blst_p1* commitments, const Fr* hx, size_t n, size_t count) {
    namespace pg = kzgamd::pairing_gpu;
    const size_t np = 2 * count;
    hipStream_t st = kz->st;
    kz->gjac.ensure(np * sizeof(blst_p1));
    kz->aff.ensure(np * sizeof(AffPt));
    kz->pref.ensure(np * sizeof(fp28::Fe));
    kz->stat.ensure(2 * sizeof(int));
    kz->gflags.ensure(np);
    kz->gsplit.ensure(count * sizeof(kzgamd::RootSplit));
    kz->gxyzz.ensure(count * sizeof(Xyzz));
    kz->gprod.ensure(count * sizeof(Xyzz));
    kz->gtab.ensure(18 * count * sizeof(Xyzz));
    kz->gsum.ensure(count * sizeof(blst_p1));
    kz->gok.ensure(count);
    ff::Fp* jac = kz->gjac.as<ff::Fp>();  // [proofs | commitments]
    int* stat = kz->stat.as<int>();
    DEV_TRY(hipMemcpyAsync(jac, proofs, count * sizeof(blst_p1), hipMemcpyHostToDevice, st));
    DEV_TRY(hipMemcpyAsync(jac + 3 * count, commitments, count * sizeof(blst_p1), hipMemcpyHostToDevice, st));
    DEV_TRY(hipMemsetAsync(stat, 0, 2 * sizeof(int), st));
    hipLaunchKernelGGL(k_kzg_points, dim3(blocks(blocks(np, PT_CHUNK), 64)), dim3(64), 0, st, kz->aff.as<AffPt>(), (const ff::Fp*)jac,
                       kz->pref.as<fp28::Fe>(), np, stat);
    hipLaunchKernelGGL(k_kzg_in_g1_each, dim3(blocks(np, 64)), dim3(64), 0, st, (const AffPt*)kz->aff.as<AffPt>(), np,
                       kz->gflags.as<uint8_t>());
    DEV_TRY(hipGetLastError());
    int hstat[2] = {1, 1};
    std::vector<uint8_t> flags(np);
    DEV_TRY(hipMemcpyAsync(hstat, stat, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    DEV_TRY(hipMemcpyAsync(flags.data(), kz->gflags.p, np, hipMemcpyDeviceToHost, st));
    DEV_TRY(hipStreamSynchronize(st));
    if (hstat[0]) return false;
    to_host.assign(count, 0);
    std::vector<kzgamd::RootSplit> split(count);
    size_t taken = 0;
    for (size_t t = 0; t < count; ++t) {
        const ff::Fp* P = reinterpret_cast<const ff::Fp*>(&proofs[t]);
        const ff::Fp* Cm = reinterpret_cast<const ff::Fp*>(&commitments[t]);
        kzgamd::RootSplit rs;
        memset(&rs, 0, sizeof rs);
        if (!flags[t] || !flags[count + t] || P[2].is_zero() || Cm[2].is_zero()) {
            to_host[t] = 1;  // its scalar stays zero: the lane gives the identity
        } else {
            Fr xn = hx[t];
            for (size_t m = 1; m < n; m <<= 1) xn = ff::mul(xn, xn);
            xn = ff::from_mont(xn);
            u32 k1[8], k2[8];
            kzgamd::glv_split(xn.v, k1, k2, rs.neg[0], rs.neg[1]);
            for (int i = 0; i < 4; ++i) {
                rs.k[0][i] = k1[i];
                rs.k[1][i] = k2[i];
            }
            ++taken;
        }
        split[t] = rs;
    }
    verdict.assign(count, 0);
    if (taken == 0) return true;
    if (!kz->have_dgen) {
        const kzgamd::pairing::G2Jac gen = kzgamd::pairing::g2_generator();
        blst_p2 g;
        memcpy(&g, &gen, sizeof g);
        DEV_TRY(pg::device_table(&kz->dgen, &g));
        kz->have_dgen = true;
    }
    auto it = kz->dlines.find(n);
    if (it == kz->dlines.end()) {
        blst_p2 q;
        memcpy(&q, &kz->g2[n], sizeof q);
        pg::DeviceTable tab;
        DEV_TRY(pg::device_table(&tab, &q));
        it = kz->dlines.emplace(n, tab).first;
    }
    DEV_TRY(hipMemcpyAsync(kz->gsplit.p, split.data(), count * sizeof(kzgamd::RootSplit), hipMemcpyHostToDevice, st));
    kzgamd::g1_jacobian_to_xyzz(kz->gxyzz.p, jac, count, st);
    kzgamd::g1_varmul_sum_device(kz->ntt, kz->gprod.p, nullptr, kz->gtab.p, kz->gxyzz.p, count, (const kzgamd::RootSplit*)kz->gsplit.p, count, 1,
                                 st);
    hipLaunchKernelGGL(k_kzg_g1_add_xyzz, dim3(blocks(count, 64)), dim3(64), 0, st, kz->gsum.as<ff::Fp>(), dif, (const Xyzz*)kz->gprod.p,
                       count);
    DEV_TRY(hipGetLastError());
    DEV_TRY(pg::check_on_stream(kz->gok.as<uint8_t>(), (const blst_p1*)kz->gsum.p, (const blst_p1*)jac, kz->dgen, it->second, count, st));
    DEV_TRY(hipMemcpyAsync(verdict.data(), kz->gok.p, count, hipMemcpyDeviceToHost, st));
    DEV_TRY(hipStreamSynchronize(st));
    return true;
}

// kzgamd_kzg_check: one pairing per tuple (also what check_batch fills ok_each with when a batch fails)
int check_each(KzgCtx* kz, bool* ok, const blst_p1* commitments, const blst_p1* proofs, const blst_fr* xs, const blst_fr* ys, size_t n,
               size_t count) {
    namespace pr = kzgamd::pairing;
    if (!kz) return -1;
    if (n == 0 || (n & (n - 1))) return 3;
    if (n > kz->ntt->W) return 4;
    if (kz->num_g2 <= n) return 6;
    if (n > kz->num_g1) return 1;
    if (count == 0) return 0;
    if (!ok || !commitments || !proofs || !xs || !ys) return -1;
    const Fr* hx = reinterpret_cast<const Fr*>(xs);
    if (n > 1)
        for (size_t i = 0; i < count; ++i)
            if (hx[i].is_zero()) return 5;
    std::vector<blst_p1> lhs(count);
    // the GPU form: verdict bytes of the tuples it took, and which tuples stay with the host loop
    bool gpu = kz->pairing_gpu_min != 0 && count >= kz->pairing_gpu_min;
    std::vector<uint8_t> gverdict, to_host;
    const int rc = kzgamd::run_call(kz, [&] {
        kz->r.ensure(count * n * sizeof(Fr));
        kz->r2.ensure(count * n * sizeof(Fr));
        kz->xs.ensure(count * sizeof(Fr));
        kz->out.ensure(count * sizeof(blst_p1));
        kz->pts.ensure(2 * count * sizeof(blst_p1));
        hipStream_t st = kz->st;
        ff::Fp* com = kz->pts.as<ff::Fp>();
        ff::Fp* dif = com + 3 * count;
        DEV_TRY(hipMemcpyAsync(kz->r.p, ys, count * n * sizeof(Fr), hipMemcpyHostToDevice, st));
        DEV_TRY(hipMemcpyAsync(com, commitments, count * sizeof(blst_p1), hipMemcpyHostToDevice, st));
        const Fr* interp = kz->r.as<Fr>();
        if (n > 1) {
            // interp = ifft(ys); interp[i] *= x^-i (kzg_settings.rs:248-258)
            DEV_TRY(hipMemcpyAsync(kz->xs.p, xs, count * sizeof(Fr), hipMemcpyHostToDevice, st));
            if (kzgamd_ntt_fr_device(kz->ntt, kz->r2.p, kz->r.p, n, count, 1, st) != 0) throw DevErr{hipErrorUnknown};
            hipLaunchKernelGGL(k_kzg_invert, dim3(blocks(count, 64)), dim3(64), 0, st, kz->xs.as<Fr>(), count);
            hipLaunchKernelGGL(k_kzg_unscale, dim3(blocks(count * n)), dim3(256), 0, st, kz->r2.as<Fr>(), kz->xs.as<Fr>(), n,
                               count * n);
            interp = kz->r2.as<Fr>();
        }
        msm_on_stream(kz, kz->out.p, interp, n, count);
        hipLaunchKernelGGL(k_kzg_g1_sub, dim3(blocks(count, 64)), dim3(64), 0, st, dif, (const ff::Fp*)com,
                           (const ff::Fp*)kz->out.p, count);
        DEV_TRY(hipGetLastError());
        DEV_TRY(hipMemcpyAsync(lhs.data(), dif, count * sizeof(blst_p1), hipMemcpyDeviceToHost, st));
        if (gpu) gpu = check_each_gpu(kz, gverdict, to_host, (const ff::Fp*)dif, proofs, commitments, hx, n, count);
    });
    if (rc) return rc;
    // the G2 side and the pairings, on the host like the reference's:  e(lhs, G2) == e(proof, [s^n]G2 - [x^n]G2)
    const pr::G2Jac gen = pr::g2_generator();
    const std::shared_ptr<const pr::LineTable> tgen = pr::prepared_lines(gen);
    for (size_t i = 0; i < count; ++i) {
        if (gpu && !to_host[i]) {
            ok[i] = gverdict[i] != 0;
            continue;
        }
        Fr xn = hx[i];
        for (size_t m = 1; m < n; m <<= 1) xn = ff::mul(xn, xn);
        xn = ff::from_mont(xn);
        const pr::G2Jac rhs2 = pr::g2_add(kz->g2[n], pr::g2_neg(pr::g2_mul(gen, xn.v)));
        const pr::LineTable trhs = pr::g2_line_table(pr::g2_to_affine(rhs2));
        ff::Fp px[2], py[2];
        bool inf[2];
        inf[0] = kzgamd::host_p1_to_affine(&lhs[i], px[0], py[0]);
        inf[1] = kzgamd::host_p1_to_affine(&proofs[i], px[1], py[1]);
        if (!inf[0]) py[0] = hfp::neg(py[0]);  // e(-lhs, G2) e(proof, rhs2) == 1
        const pr::LineTable* tabs[2] = {tgen.get(), &trhs};
        ok[i] = pr::f12_is_one(pr::final_exponentiation(pr::miller_loop_multi(tabs, px, py, inf, 2)));
    }
    return 0;
}

// D = "KZGAMD_CHKBATCH1" | u64_be(n) | u64_be(count) | commitments | proofs | xs | ys, the caller's bytes;
// r = the SHA-256 of D as a big-endian integer mod the group order (hash_to_bls_field), Montgomery form
Fr batch_challenge(const blst_p1* commitments, const blst_p1* proofs, const blst_fr* xs, const blst_fr* ys, size_t n, size_t count) {
    kzgamd::Sha256 h;
    uint8_t head[32];
    memcpy(head, "KZGAMD_CHKBATCH1", 16);
    for (int i = 0; i < 8; ++i) {
        head[16 + 7 - i] = (uint8_t)((uint64_t)n >> (8 * i));
        head[24 + 7 - i] = (uint8_t)((uint64_t)count >> (8 * i));
    }
    h.update(head, 32);
    if (count) {
        h.update((const uint8_t*)commitments, count * sizeof(blst_p1));
        h.update((const uint8_t*)proofs, count * sizeof(blst_p1));
        h.update((const uint8_t*)xs, count * sizeof(blst_fr));
        if (n) h.update((const uint8_t*)ys, count * n * sizeof(blst_fr));
    }
    uint8_t digest[32];
    h.finish(digest);
    Fr v;
    for (int i = 0; i < 8; ++i) {
        const uint8_t* q = digest + (7 - i) * 4;
        v.v[i] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
    }
    return ff::mul(v, Fr::r2());
}

// the argument checks the batched calls share, kzgamd_kzg_check's codes in its order; 0 = go on
int batch_args(KzgCtx* kz, bool need_g2, const void* out, const blst_p1* commitments, const blst_p1* proofs, const blst_fr* xs,
               const blst_fr* ys, size_t n, size_t count) {
    if (n == 0 || (n & (n - 1))) return 3;
    if (n > kz->ntt->W) return 4;
    if (need_g2 && kz->num_g2 <= n) return 6;
    if (n > kz->num_g1) return 1;
    if (!out) return -1;  // written even when count == 0
    if (count == 0) return 0;
    if (!commitments || !proofs || !xs || !ys) return -1;
    const Fr* hx = reinterpret_cast<const Fr*>(xs);
    if (n > 1)
        for (size_t i = 0; i < count; ++i)
            if (hx[i].is_zero()) return 5;
    return 0;
}

// L and P of the batch into lp[0], lp[1] (count > 0, arguments checked).  0 ok, 7 a point off the curve or outside G1,
// negative = device error.  r: the weight base (the caller's, or the challenge hashed before the lock was taken).
// tab_n != nullptr: also look up (or build) the line table of [s^n]G2, under the same lock.
int batch_g1(KzgCtx* kz, blst_p1 lp[2], const blst_p1* commitments, const blst_p1* proofs, const blst_fr* xs, const blst_fr* ys,
             size_t n, size_t count, const Fr& r, std::shared_ptr<const kzgamd::pairing::LineTable>* tab_n) {
    namespace pr = kzgamd::pairing;
    const size_t np = 2 * count, nblocks = blocks(count, AGG_WAVE);
    return kzgamd::run_call(kz, [&]() -> int {
        kz->pts.ensure(np * sizeof(blst_p1));
        kz->aff.ensure(np * sizeof(AffPt));
        kz->pref.ensure(np * sizeof(fp28::Fe));
        kz->stat.ensure(2 * sizeof(int));
        kz->r.ensure(count * n * sizeof(Fr));
        if (n > 1) kz->r2.ensure(count * n * sizeof(Fr));
        kz->xs.ensure((count + 1) * sizeof(Fr));  // the x of every tuple, then r
        if (n > 1) kz->xinv.ensure(count * sizeof(Fr));
        kz->rho.ensure(count * sizeof(Fr));
        kz->rows.ensure(2 * np * sizeof(Fr));
        kz->part.ensure(nblocks * n * sizeof(Fr));
        kz->agg.ensure(n * sizeof(Fr));
        kz->out.ensure(4 * sizeof(blst_p1));  // L | P | row L | [A(s)]G
        hipStream_t st = kz->st;
        ff::Fp* jac = kz->pts.as<ff::Fp>();
        AffPt* aff = kz->aff.as<AffPt>();
        int* stat = kz->stat.as<int>();
        Fr* dx = kz->xs.as<Fr>();
        ff::Fp* out = kz->out.as<ff::Fp>();
        int hstat[2] = {1, 1};
        // points: [proofs | commitments] -> affine slots, on the curve, in G1
        DEV_TRY(hipMemcpyAsync(jac, proofs, count * sizeof(blst_p1), hipMemcpyHostToDevice, st));
        DEV_TRY(hipMemcpyAsync(jac + 3 * count, commitments, count * sizeof(blst_p1), hipMemcpyHostToDevice, st));
        DEV_TRY(hipMemsetAsync(stat, 0, 2 * sizeof(int), st));
        hipLaunchKernelGGL(k_kzg_points, dim3(blocks(blocks(np, PT_CHUNK), 64)), dim3(64), 0, st, aff, (const ff::Fp*)jac,
                           kz->pref.as<fp28::Fe>(), np, stat);
        hipLaunchKernelGGL(k_kzg_in_g1, dim3(blocks(np, 64)), dim3(64), 0, st, (const AffPt*)aff, np, stat);
        // values: the inverse transforms and x^-1
        DEV_TRY(hipMemcpyAsync(kz->r.p, ys, count * n * sizeof(Fr), hipMemcpyHostToDevice, st));
        DEV_TRY(hipMemcpyAsync(dx, xs, count * sizeof(Fr), hipMemcpyHostToDevice, st));
        const Fr* vals = kz->r.as<Fr>();
        if (n > 1) {
            if (kzgamd_ntt_fr_device(kz->ntt, kz->r2.p, kz->r.p, n, count, 1, st) != 0) throw DevErr{hipErrorUnknown};
            DEV_TRY(hipMemcpyAsync(kz->xinv.p, dx, count * sizeof(Fr), hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(k_kzg_invert, dim3(blocks(count, 64)), dim3(64), 0, st, kz->xinv.as<Fr>(), count);
            vals = kz->r2.as<Fr>();
        }
        DEV_TRY(hipGetLastError());
        DEV_TRY(hipMemcpyAsync(hstat, stat, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        DEV_TRY(hipStreamSynchronize(st));
        if (hstat[0] || hstat[1]) return 7;
        // the checked points become the bases of the variable-base handle (all in G1: the GLV split holds)
        if (!kz->vmsm) kz->vmsm = kzgamd::msm_create(aff, np, true, false, true, kzgamd::G1_TRUSTED, &kz->opt);
        else kzgamd::msm_reset_points(kz->vmsm, aff, np);
        DEV_TRY(hipMemcpyAsync(dx + count, &r, sizeof(Fr), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_kzg_batch_scalars, dim3(blocks(count, 64)), dim3(64), 0, st, kz->rho.as<Fr>(), kz->rows.as<Fr>(),
                           (const Fr*)(dx + count), (const Fr*)dx, n, count);
        Fr* part = nblocks > 1 ? kz->part.as<Fr>() : kz->agg.as<Fr>();
        hipLaunchKernelGGL(k_kzg_batch_agg, dim3((unsigned)nblocks), dim3(AGG_WAVE), 0, st, part, vals, (const Fr*)kz->rho.as<Fr>(),
                           n > 1 ? (const Fr*)kz->xinv.as<Fr>() : (const Fr*)nullptr, n, count);
        if (nblocks > 1)
            hipLaunchKernelGGL(k_kzg_batch_fold, dim3(blocks(n)), dim3(256), 0, st, kz->agg.as<Fr>(), (const Fr*)part, n, nblocks);
        DEV_TRY(hipGetLastError());
        msm_on_stream(kz, out + 9, kz->agg.p, n, 1);  // [A(s)]G
        {
            kzgamd::MsmLock locked(kz->vmsm);
            kzgamd::msm_enqueue(kz->vmsm, out + 3, kz->rows.p, np, 2, 1, st, kzgamd::OUT_JACOBIAN);  // P, row L
        }
        hipLaunchKernelGGL(k_kzg_g1_sub, dim3(1), dim3(64), 0, st, out, (const ff::Fp*)(out + 6), (const ff::Fp*)(out + 9), (size_t)1);
        DEV_TRY(hipGetLastError());
        DEV_TRY(hipMemcpyAsync(lp, out, 2 * sizeof(blst_p1), hipMemcpyDeviceToHost, st));
        if (tab_n) {
            auto it = kz->lines.find(n);
            if (it == kz->lines.end())
                it = kz->lines.emplace(n, std::make_shared<const pr::LineTable>(pr::g2_line_table(pr::g2_to_affine(kz->g2[n])))).first;
            *tab_n = it->second;
        }
        return 0;
    });
}

}  // namespace

extern "C" int kzgamd_kzg_check(void* vkz, bool* ok, const blst_p1* commitments, const blst_p1* proofs, const blst_fr* xs,
                                const blst_fr* ys, size_t n, size_t count) {
    return check_each((KzgCtx*)vkz, ok, commitments, proofs, xs, ys, n, count);
}

extern "C" int kzgamd_kzg_batch_challenge(blst_fr* r_out, const blst_p1* commitments, const blst_p1* proofs, const blst_fr* xs,
                                          const blst_fr* ys, size_t n, size_t count) {
    if (!r_out || (count && (!commitments || !proofs || !xs || (n && !ys)))) return -1;
    const Fr r = batch_challenge(commitments, proofs, xs, ys, n, count);
    memcpy(r_out, &r, sizeof r);
    return 0;
}

extern "C" int kzgamd_kzg_check_batch_g1(void* vkz, blst_p1 out[2], const blst_p1* commitments, const blst_p1* proofs,
                                         const blst_fr* xs, const blst_fr* ys, size_t n, size_t count, const blst_fr* r) {
    KzgCtx* kz = (KzgCtx*)vkz;
    if (!kz) return -1;
    if (const int rc = batch_args(kz, false, out, commitments, proofs, xs, ys, n, count)) return rc;
    if (count == 0) {
        memset(out, 0, 2 * sizeof(blst_p1));
        return 0;
    }
    // the hash of 2 count points and count (n + 1) scalars runs BEFORE the handle's lock is taken: other callers of the
    // handle are not held up by it
    const Fr w = r ? *reinterpret_cast<const Fr*>(r) : batch_challenge(commitments, proofs, xs, ys, n, count);
    blst_p1 lp[2];
    const int rc = batch_g1(kz, lp, commitments, proofs, xs, ys, n, count, w, nullptr);
    if (rc == 0) memcpy(out, lp, sizeof lp);
    return rc;
}

extern "C" int kzgamd_kzg_check_batch(void* vkz, bool* ok, bool* ok_each, const blst_p1* commitments, const blst_p1* proofs,
                                      const blst_fr* xs, const blst_fr* ys, size_t n, size_t count, const blst_fr* r) {
    namespace pr = kzgamd::pairing;
    KzgCtx* kz = (KzgCtx*)vkz;
    if (!kz) return -1;
    if (const int rc = batch_args(kz, true, ok, commitments, proofs, xs, ys, n, count)) return rc;
    if (count == 0) {
        *ok = true;
        return 0;
    }
    const Fr w = r ? *reinterpret_cast<const Fr*>(r) : batch_challenge(commitments, proofs, xs, ys, n, count);  // before the lock
    blst_p1 lp[2];
    std::shared_ptr<const pr::LineTable> tab_n;
    if (const int rc = batch_g1(kz, lp, commitments, proofs, xs, ys, n, count, w, &tab_n)) return rc;
    const std::shared_ptr<const pr::LineTable> tab_gen = pr::prepared_lines(pr::g2_generator());
    // one pairing check, outside the handle's lock:  e(-L, G2) e(P, [s^n]G2) == 1
    ff::Fp px[2], py[2];
    bool inf[2];
    inf[0] = kzgamd::host_p1_to_affine(&lp[0], px[0], py[0]);
    inf[1] = kzgamd::host_p1_to_affine(&lp[1], px[1], py[1]);
    if (!inf[0]) py[0] = hfp::neg(py[0]);
    const pr::LineTable* tabs[2] = {tab_gen.get(), tab_n.get()};
    const bool pass = pr::f12_is_one(pr::final_exponentiation(pr::miller_loop_multi(tabs, px, py, inf, 2)));
    if (ok_each) {
        if (pass) {
            for (size_t i = 0; i < count; ++i) ok_each[i] = true;
        } else if (const int rc = check_each(kz, ok_each, commitments, proofs, xs, ys, n, count)) {
            return rc;
        }
    }
    *ok = pass;
    return 0;
}
