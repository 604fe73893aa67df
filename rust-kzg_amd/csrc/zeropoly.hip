// Zero polynomials and sample recovery over Fr: the reference's ZeroPoly (blst/src/zero_poly.rs: do_zero_poly_mul_partial,
// reduce_partials, zero_poly_via_multiplication) and PolyRecover (blst/src/recovery.rs: recover_poly_coeffs_from_samples,
// recover_poly_from_samples) on the handle of kzgamd_poly_new, several problems per call.  Every output is a field
// element with one value (a monic product of linear factors, its transform, a pointwise quotient by a value that is
// never zero), so whichever route runs gives the reference's elements exactly; the reference's own route (partials of
// 256, reduction by 4, serial long multiplication) is not imitated.  Nothing is serial in the polynomial's length beyond
// the 64 roots of one wave: a dependent Fr multiplication is ~1.1 us on a lone wave (profiles/NOTES.md).
//
//   Z = prod (X - w^idx) is kept WITHOUT its leading 1: a product of `count` roots is `count` low coefficients, and the
//   products of one problem lie back to back in one array of `count` elements (polynomial j of a level with d
//   coefficients each at j d; the last may be shorter).  A level therefore rewrites its pairs in place and an odd
//   polynomial stays where it is.
//   leaf     one wave per group of <= 64 roots of one problem (k_zp_leaf): lane j keeps coefficient j, each root is one
//            step c_j <- c_{j-1} - w c_j with the neighbour fetched by shuffle.  1 launch for every problem of the call.
//   tree     level l multiplies neighbouring pairs of d = 64 2^l coefficients of every problem of the call:
//            (X^d + a)(X^e + b) = X^(d+e) + [X^d b + X^e a + a b], e <= d.  The bracket has d + e <= 2d coefficients, so
//            a transform of N = 2d (not 4d) holds it without wrap: k_zp_pad writes a and b zero-padded to N, one forward
//            transform of 2 x pairs lists, k_zp_pointwise forms A B + w^(d i) B + w^(e i) A (w^(d i) = +-1), one inverse
//            transform of pairs lists, k_zp_cut writes the d + e coefficients back.  3 launches and 2 batched
//            transforms a level, ceil(log2(ceil(count / 64))) levels (kzgamd_poly_zero_plan).  The shorter last
//            polynomial and problems of different counts are entries of the pair table, not padding roots.
//   direct   one lane per (problem, domain point t) multiplies out Z(w^t) over the problem's list (k_zp_direct); one
//            inverse transform gives the coefficients.  Form 0 takes it while the longest list of the call has at most
//            ZP_DIRECT_MAX roots: 0, since the tree was level or ahead at every measured size.  It is the forced form 1,
//            an independent route to the same elements.
//   reduce_partials   every partial zero-padded to N = next_pow2(output length), one forward transform of all of them,
//            log2(npartial) halving launches of pointwise products, one inverse transform.
//   recover  Z and fft Z by the above; k_rc_mask (E . fft Z, a missing sample is never read); one inverse transform;
//            k_rc_shift applies 5^-i to it and to Z; one forward transform of 2 nprob lists; k_rc_div; one inverse
//            transform; k_rc_scale applies 5^i; for the evaluation form one more forward transform.  The powers are
//            square-and-multiply on the public exponent per lane.  k_rc_div inverts per lane (ff::inverse_bgcd): one
//            inversion per wave over a product scan measured the same and was dropped (profiles/NOTES.md §30).
// Wave-local exchange and global memory between launches only: no workgroup barrier in this file, and no workgroup
// depends on another within a launch.  A call holds the handle's lock, runs on its stream, is sliced when its workspace
// would take more than the share of the free HBM the other kzgamd_poly_* calls allow, and synchronises before it returns.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

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

constexpr size_t LEAF = 64;            // roots a wave of the leaf kernel takes: a lane each
constexpr size_t ZP_DIRECT_MAX = 0;   // form 0: the direct form while no list of the call is longer — never: it was not
                                       // ahead at any measured size (profiles/NOTES.md §30); it stays as the forced form 1

typedef unsigned long long u64;

// an entry of a plan table: a run of `len` elements at `off` (a leaf group, the second polynomial of a pair, a problem)
struct ZSpan {
    u64 off;
    u32 len, pad;
};

// a wave per group of <= 64 roots: c[off + j] = coefficient j of prod_k (X - roots[idx[off + k] * rs]) below its leading 1
__global__ void __launch_bounds__(64) k_zp_leaf(Fr* __restrict__ c, const u64* __restrict__ idx, const Fr* __restrict__ roots, size_t rs,
                                                const ZSpan* __restrict__ groups) {
    const ZSpan g = groups[blockIdx.x];
    const u32 lane = threadIdx.x;
    const Fr w = lane < g.len ? roots[idx[g.off + lane] * rs] : Fr::zero();
    Fr cl = Fr::zero();
    for (u32 k = 0; k < g.len; ++k) {
        const Fr wk = shfl_idx(w, (int)k);
        if (lane == k) cl = Fr::one();  // the leading coefficient of the product so far
        Fr up = shfl_up(cl, 1);
        if (lane == 0) up = Fr::zero();
        const Fr nv = ff::sub(up, fr_mul(wk, cl));
        if (lane <= k) cl = nv;
    }
    if (lane < g.len) c[g.off + lane] = cl;
}

// pair p = (a: d coefficients at pairs[p].off, b: pairs[p].len coefficients at off + d):
// f[(2p) N + i] = a_i, f[(2p + 1) N + i] = b_i, zeros up to N = 2d
__global__ void __launch_bounds__(256) k_zp_pad(Fr* __restrict__ f, const Fr* __restrict__ c, const ZSpan* __restrict__ pairs, size_t d,
                                                size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t N = 2 * d, p = t / (2 * N), r = t % (2 * N);
    const ZSpan pr = pairs[p];
    Fr v = Fr::zero();
    if (r < N) {
        if (r < d) v = c[pr.off + r];
    } else if (r - N < pr.len) {
        v = c[pr.off + d + (r - N)];
    }
    f[t] = v;
}

// dst[p N + i] = A B + w^(d i) B + w^(e i) A at the N-th root w = roots[rsN]: the transform of X^d b + X^e a + a b
__global__ void __launch_bounds__(256) k_zp_pointwise(Fr* __restrict__ dst, const Fr* __restrict__ src, const ZSpan* __restrict__ pairs,
                                                      const Fr* __restrict__ roots, size_t rsN, size_t d, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t N = 2 * d, p = t / N, i = t % N;
    const size_t e = pairs[p].len;
    const Fr A = src[2 * p * N + i], B = src[(2 * p + 1) * N + i];
    Fr r = fr_mul(A, B);
    r = (i & 1) ? ff::sub(r, B) : ff::add(r, B);
    if (e == d) r = (i & 1) ? ff::sub(r, A) : ff::add(r, A);
    else r = ff::add(r, fr_mul(roots[((e * i) & (N - 1)) * rsN], A));
    dst[t] = r;
}

// c[off + r] = src[p N + r], r < d + e
__global__ void __launch_bounds__(256) k_zp_cut(Fr* __restrict__ c, const Fr* __restrict__ src, const ZSpan* __restrict__ pairs, size_t d,
                                                size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t N = 2 * d, p = t / N, r = t % N;
    const ZSpan pr = pairs[p];
    if (r < d + pr.len) c[pr.off + r] = src[t];
}

// zp[b n + i] = c[probs[b].off + i] (i < count), 1 (i == count), 0 beyond
__global__ void __launch_bounds__(256) k_zp_expand(Fr* __restrict__ zp, const Fr* __restrict__ c, const ZSpan* __restrict__ probs, size_t n,
                                                   size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t b = t / n, i = t % n;
    const ZSpan pr = probs[b];
    zp[t] = i < pr.len ? c[pr.off + i] : (i == pr.len ? Fr::one() : Fr::zero());
}

// ze[b n + t] = prod_k (roots[t rs] - roots[idx[off + k] rs])
__global__ void __launch_bounds__(256) k_zp_direct(Fr* __restrict__ ze, const u64* __restrict__ idx, const ZSpan* __restrict__ probs,
                                                   const Fr* __restrict__ roots, size_t rs, size_t n, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t b = t / n, i = t % n;
    const ZSpan pr = probs[b];
    const Fr x = roots[i * rs];
    Fr acc = Fr::one();
    for (u32 k = 0; k < pr.len; ++k) acc = fr_mul(acc, ff::sub(x, roots[idx[pr.off + k] * rs]));
    ze[t] = acc;
}

// f[s N + i] = coefficient i of partial s (spans[s]: where it starts in `parts`, its length), zeros up to N
__global__ void __launch_bounds__(256) k_rp_pad(Fr* __restrict__ f, const Fr* __restrict__ parts, const ZSpan* __restrict__ spans, size_t N,
                                                size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t s = t / N, i = t % N;
    const ZSpan sp = spans[s];
    f[t] = i < sp.len ? parts[sp.off + i] : Fr::zero();
}

// g[k N + i] *= g[(k + half) N + i] for k < half, k + half < m
__global__ void __launch_bounds__(256) k_rp_fold(Fr* __restrict__ g, size_t m, size_t half, size_t N, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t k = t / N;
    if (k + half < m) g[t] = fr_mul(g[t], g[t + half * N]);
}

// acc[i] *= g[i]
__global__ void __launch_bounds__(256) k_rp_acc(Fr* __restrict__ acc, const Fr* __restrict__ g, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < total) acc[t] = fr_mul(acc[t], g[t]);
}

// dst[t] = samples[t] * ze[t] where the sample is present, 0 where it is missing (its value is not read)
__global__ void __launch_bounds__(256) k_rc_mask(Fr* __restrict__ dst, const Fr* __restrict__ samples, const uint8_t* __restrict__ present,
                                                 const Fr* __restrict__ ze, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    dst[t] = present[t] ? fr_mul(samples[t], ze[t]) : Fr::zero();
}

// f[(2b) n + i] = u[b n + i] k^i, f[(2b + 1) n + i] = zp[b n + i] k^i
__global__ void __launch_bounds__(256) k_rc_shift(Fr* __restrict__ f, const Fr* __restrict__ u, const Fr* __restrict__ zp, Fr k, size_t n,
                                                  size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t b = t / (2 * n), r = t % (2 * n);
    const size_t i = r < n ? r : r - n;
    const Fr v = r < n ? u[b * n + i] : zp[b * n + i];
    f[t] = fr_mul(v, fr_pow(k, i));
}

// a[t] *= k^(t mod n): the exponent is i, not the i + 1 of Poly::scale
__global__ void __launch_bounds__(256) k_rc_scale(Fr* __restrict__ a, Fr k, size_t n, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    a[t] = fr_mul(a[t], fr_pow(k, t % n));
}

// q[b n + i] = g[(2b) n + i] / g[(2b + 1) n + i]; the divisor is never zero (5 is not a 2^k-th root of unity)
__global__ void __launch_bounds__(256) k_rc_div(Fr* __restrict__ q, const Fr* __restrict__ g, size_t n, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const size_t b = t / n, i = t % n;
    q[t] = fr_mul(g[2 * b * n + i], ff::inverse_bgcd(g[(2 * b + 1) * n + i]));
}

// ---- host side ----

// the tree over `count` roots: level l has d = LEAF 2^l coefficients per polynomial while d < count
size_t zero_levels(size_t count) {
    size_t l = 0;
    for (size_t d = LEAF; d < count && d; d <<= 1) ++l;
    return l;
}
// the longest transform the tree over `count` roots runs (0: none)
size_t zero_max_transform(size_t count) {
    const size_t l = zero_levels(count);
    return l ? 2 * (LEAF << (l - 1)) : 0;
}

// the tables of one slice of problems, as one array for one copy: problems, leaf groups, then the pairs level by level
struct ZeroPlan {
    std::vector<ZSpan> tab;
    size_t nprob = 0, ngroup = 0, total = 0;
    std::vector<size_t> level_at, level_n;  // where a level's pairs start in tab, how many
    size_t work = 0;                        // max over the levels of pairs x N: elements of a transform buffer / 2
    size_t maxcount = 0;
};
// problem b of the slice has `counts(b)` roots; its roots and its coefficients start at the sum of the counts before it
template <class CountOf>
void zero_plan_build(ZeroPlan& pl, size_t nprob, CountOf counts) {
    pl.tab.clear();
    pl.level_at.clear();
    pl.level_n.clear();
    pl.nprob = nprob;
    pl.work = pl.maxcount = 0;
    size_t off = 0;
    for (size_t b = 0; b < nprob; ++b) {
        const size_t cnt = counts(b);
        pl.tab.push_back(ZSpan{(u64)off, (u32)cnt, 0});
        if (cnt > pl.maxcount) pl.maxcount = cnt;
        off += cnt;
    }
    pl.total = off;
    for (size_t b = 0; b < nprob; ++b) {
        const ZSpan pr = pl.tab[b];
        for (size_t j = 0; j < pr.len; j += LEAF) pl.tab.push_back(ZSpan{pr.off + j, (u32)min_sz(LEAF, pr.len - j), 0});
    }
    pl.ngroup = pl.tab.size() - nprob;
    const size_t nlev = zero_levels(pl.maxcount);
    for (size_t l = 0; l < nlev; ++l) {
        const size_t d = LEAF << l;
        pl.level_at.push_back(pl.tab.size());
        for (size_t b = 0; b < nprob; ++b) {
            const ZSpan pr = pl.tab[b];
            for (size_t j = 0; j + d < pr.len; j += 2 * d) pl.tab.push_back(ZSpan{pr.off + j, (u32)min_sz(d, pr.len - j - d), 0});
        }
        pl.level_n.push_back(pl.tab.size() - pl.level_at.back());
        if (pl.level_n.back() * 2 * d > pl.work) pl.work = pl.level_n.back() * 2 * d;
    }
}

// a transform on the handle's stream; a list of one element is its own transform
void zntt(PolyCtx* pc, Fr* out, const Fr* in, size_t n, size_t nbatch, int inverse) {
    if (n == 1) DEV_TRY(hipMemcpyAsync(out, in, nbatch * sizeof(Fr), hipMemcpyDeviceToDevice, pc->st));
    else ntt_on_stream(pc, out, in, n, nbatch, inverse);
}

void ensure_roots(PolyCtx* pc) {
    if (pc->roots_ready) return;
    const size_t bytes = (pc->ntt->W + 1) * sizeof(Fr);
    pc->roots.ensure(bytes);
    upload(pc, pc->roots.p, pc->ntt->roots.data(), bytes);
    pc->roots_ready = true;
}

// workspace of a zero-polynomial computation of the plan's slice besides its outputs: idx, tab, zc; f and g for the tree
void zero_reserve(PolyCtx* pc, const ZeroPlan& pl, bool direct, size_t min_fg) {
    pc->idx.ensure((pl.total ? pl.total : 1) * sizeof(u64));
    pc->tab.ensure(pl.tab.size() * sizeof(ZSpan));
    pc->zc.ensure((pl.total ? pl.total : 1) * sizeof(Fr));
    size_t fg = direct ? 0 : 2 * pl.work;
    if (fg < min_fg) fg = min_fg;
    if (fg) {
        pc->f.ensure(fg * sizeof(Fr));
        pc->g.ensure(fg * sizeof(Fr));
    }
}

// Enqueues the products of the plan's problems from idx_host[0 .. pl.total) (root index k of the list times rs into
// roots[]): zp[b n + i] = coefficient i (leading 1 included, zeros up to n) and / or ze = the forward transform of
// length n of it.  zp may be NULL only in the tree form without ze; in the direct form ze is computed first and must
// not be NULL (n is then a power of two).  pl.tab and idx_host must stay alive until the stream is synchronised.
void enqueue_zero(PolyCtx* pc, Fr* zp, Fr* ze, size_t n, size_t rs, const ZeroPlan& pl, const u64* idx_host, bool direct, bool want_zp) {
    hipStream_t st = pc->st;
    ensure_roots(pc);
    if (pl.total) upload(pc, pc->idx.p, idx_host, pl.total * sizeof(u64));
    upload(pc, pc->tab.p, pl.tab.data(), pl.tab.size() * sizeof(ZSpan));
    const ZSpan* tab = pc->tab.as<ZSpan>();
    const u64* idx = pc->idx.as<u64>();
    const Fr* roots = pc->roots.as<Fr>();
    const size_t total = pl.nprob * n;
    if (direct) {
        hipLaunchKernelGGL(k_zp_direct, dim3(blocks(total)), dim3(256), 0, st, ze, idx, tab, roots, rs, n, total);
        DEV_TRY(hipGetLastError());
        if (want_zp) zntt(pc, zp, ze, n, pl.nprob, 1);
        return;
    }
    Fr *c = pc->zc.as<Fr>(), *f = pc->f.as<Fr>(), *g = pc->g.as<Fr>();
    if (pl.ngroup) hipLaunchKernelGGL(k_zp_leaf, dim3((unsigned)pl.ngroup), dim3(64), 0, st, c, idx, roots, rs, tab + pl.nprob);
    for (size_t l = 0; l < pl.level_n.size(); ++l) {
        const size_t np = pl.level_n[l], d = LEAF << l, N = 2 * d;
        if (!np) continue;
        const ZSpan* pairs = tab + pl.level_at[l];
        hipLaunchKernelGGL(k_zp_pad, dim3(blocks(2 * np * N)), dim3(256), 0, st, f, (const Fr*)c, pairs, d, 2 * np * N);
        ntt_on_stream(pc, g, f, N, 2 * np, 0);
        hipLaunchKernelGGL(k_zp_pointwise, dim3(blocks(np * N)), dim3(256), 0, st, f, (const Fr*)g, pairs, roots, pc->ntt->W / N, d, np * N);
        ntt_on_stream(pc, g, f, N, np, 1);
        hipLaunchKernelGGL(k_zp_cut, dim3(blocks(np * N)), dim3(256), 0, st, c, (const Fr*)g, pairs, d, np * N);
    }
    hipLaunchKernelGGL(k_zp_expand, dim3(blocks(total)), dim3(256), 0, st, zp, (const Fr*)c, tab, n, total);
    DEV_TRY(hipGetLastError());
    if (ze) zntt(pc, ze, zp, n, pl.nprob, 0);
}

bool is_pow2(size_t v) { return v && !(v & (v - 1)); }

Fr fr_small(unsigned v) {
    Fr f = Fr::zero();
    f.v[0] = v;
    return ff::to_mont(f);
}

}  // namespace

extern "C" int kzgamd_poly_zero_info(void* vpc, size_t* leaf_roots, size_t* direct_max) {
    if (!vpc) return -1;
    if (leaf_roots) *leaf_roots = LEAF;
    if (direct_max) *direct_max = ZP_DIRECT_MAX;
    return 0;
}

extern "C" size_t kzgamd_poly_zero_plan(size_t count, size_t* levels) {
    const size_t nlev = min_sz(zero_levels(count), 32);  // more than 32 levels would need more than 2^37 roots
    if (levels)
        for (size_t l = 0; l < nlev; ++l) {
            const size_t d = LEAF << l;
            levels[3 * l] = (count + d - 1) / d;
            levels[3 * l + 1] = d;
            levels[3 * l + 2] = 2 * d;
        }
    return nlev;
}

extern "C" int kzgamd_poly_zero_partial(void* vpc, blst_fr* out, const uint64_t* idxs, size_t nidx, size_t stride) {
    PolyCtx* pc = (PolyCtx*)vpc;
    if (!pc) return -1;
    if (nidx == 0) return 1;
    if (!out || !idxs) return -1;
    const size_t W = pc->ntt->W;
    for (size_t k = 0; k < nidx; ++k)
        if (stride && idxs[k] > W / stride) return 2;
    if (zero_max_transform(nidx) > W) return 4;
    ZeroPlan pl;
    return run_call(pc, [&] {
        zero_plan_build(pl, 1, [&](size_t) { return nidx; });
        zero_reserve(pc, pl, false, 0);
        pc->out.ensure((nidx + 1) * sizeof(Fr));
        static_assert(sizeof(u64) == sizeof(uint64_t), "index width");
        enqueue_zero(pc, pc->out.as<Fr>(), nullptr, nidx + 1, stride, pl, (const u64*)idxs, false, true);
        download(pc, out, pc->out.p, (nidx + 1) * sizeof(Fr));
    });
}

extern "C" int kzgamd_poly_reduce_partials(void* vpc, blst_fr* out, size_t domain_size, const blst_fr* partials, const size_t* lens,
                                           size_t npartial) {
    PolyCtx* pc = (PolyCtx*)vpc;
    if (!pc) return -1;
    if (!is_pow2(domain_size)) return 1;
    if (npartial == 0) return 2;
    if (!out || !partials || !lens) return -1;
    size_t out_len = 1, sum = 0;
    bool too_long = false;
    for (size_t k = 0; k < npartial; ++k) {
        if (lens[k] == 0) return 5;
        sum += lens[k];
        if (out_len + (lens[k] - 1) < out_len || out_len + (lens[k] - 1) > domain_size) too_long = true;
        else out_len += lens[k] - 1;
    }
    if (too_long) return 3;
    if (domain_size > pc->ntt->W) return 4;
    const size_t N = next_pow2(out_len);  // <= domain_size
    std::vector<ZSpan> spans;
    return run_call(pc, [&] {
        const size_t per = slice_of(pc, npartial, (2 * N + sum / npartial + 1) * sizeof(Fr) + sizeof(ZSpan));
        pc->c.ensure(N * sizeof(Fr));
        pc->out.ensure(N * sizeof(Fr));
        pc->f.ensure(per * N * sizeof(Fr));
        pc->g.ensure(per * N * sizeof(Fr));
        pc->tab.ensure(per * sizeof(ZSpan));
        hipStream_t st = pc->st;
        Fr *f = pc->f.as<Fr>(), *g = pc->g.as<Fr>(), *acc = pc->c.as<Fr>();
        size_t at = 0;  // coefficients before the slice
        for (size_t done = 0; done < npartial; done += per) {
            const size_t m = min_sz(per, npartial - done);
            spans.clear();
            size_t off = 0;
            for (size_t k = 0; k < m; ++k) {
                spans.push_back(ZSpan{(u64)off, (u32)lens[done + k], 0});
                off += lens[done + k];
            }
            pc->a.ensure(off * sizeof(Fr));
            upload(pc, pc->a.p, partials + at, off * sizeof(Fr));
            upload(pc, pc->tab.p, spans.data(), m * sizeof(ZSpan));
            at += off;
            hipLaunchKernelGGL(k_rp_pad, dim3(blocks(m * N)), dim3(256), 0, st, f, pc->a.as<Fr>(), pc->tab.as<ZSpan>(), N, m * N);
            zntt(pc, g, f, N, m, 0);
            for (size_t half = next_pow2(m) / 2; half >= 1; half >>= 1)
                hipLaunchKernelGGL(k_rp_fold, dim3(blocks(half * N)), dim3(256), 0, st, g, min_sz(m, 2 * half), half, N, half * N);
            if (done == 0) DEV_TRY(hipMemcpyAsync(acc, g, N * sizeof(Fr), hipMemcpyDeviceToDevice, st));
            else hipLaunchKernelGGL(k_rp_acc, dim3(blocks(N)), dim3(256), 0, st, acc, (const Fr*)g, N);
            DEV_TRY(hipGetLastError());
            DEV_TRY(hipStreamSynchronize(st));  // the next slice rewrites `spans`
        }
        zntt(pc, pc->out.as<Fr>(), acc, N, 1, 1);
        download(pc, out, pc->out.p, out_len * sizeof(Fr));
    });
}

extern "C" int kzgamd_poly_zero_poly(void* vpc, blst_fr* zero_eval, blst_fr* zero_poly, size_t domain_size, const uint64_t* missing,
                                     const size_t* offsets, size_t nprob, int form) {
    PolyCtx* pc = (PolyCtx*)vpc;
    if (!pc || form < 0 || form > 2) return -1;
    if (nprob == 0) return 0;
    if (!offsets) return -1;
    for (size_t b = 0; b < nprob; ++b)
        if (offsets[b + 1] < offsets[b]) return -1;
    if (offsets[nprob] > offsets[0] && !missing) return -1;
    // the reference's checks in the reference's order (zero_poly.rs:191-199)
    size_t maxcount = 0;
    for (size_t b = 0; b < nprob; ++b) {
        const size_t cnt = offsets[b + 1] - offsets[b];
        if (cnt >= domain_size) return 1;
        if (cnt > maxcount) maxcount = cnt;
    }
    const size_t W = pc->ntt->W;
    if (domain_size > W) return 2;
    if (!is_pow2(domain_size)) return 3;
    for (size_t k = offsets[0]; k < offsets[nprob]; ++k)
        if (missing[k] >= domain_size) return 5;
    if (!zero_eval && !zero_poly) return 0;
    const size_t n = domain_size;
    const bool direct = form == 1 || (form == 0 && maxcount <= ZP_DIRECT_MAX);
    ZeroPlan pl;
    return run_call(pc, [&] {
        const size_t per = slice_of(pc, nprob, (10 * n + maxcount) * sizeof(Fr) + maxcount * sizeof(u64));
        pc->b.ensure(per * n * sizeof(Fr));
        pc->c.ensure(per * n * sizeof(Fr));
        for (size_t done = 0; done < nprob; done += per) {
            const size_t cnt = min_sz(per, nprob - done);
            zero_plan_build(pl, cnt, [&](size_t b) { return offsets[done + b + 1] - offsets[done + b]; });
            zero_reserve(pc, pl, direct, 0);
            Fr *zp = pc->b.as<Fr>(), *ze = pc->c.as<Fr>();
            enqueue_zero(pc, zp, (direct || zero_eval) ? ze : nullptr, n, W / n, pl, (const u64*)missing + offsets[done], direct,
                         !direct || zero_poly != nullptr);
            if (zero_poly) download(pc, zero_poly + done * n, zp, cnt * n * sizeof(Fr));
            if (zero_eval) download(pc, zero_eval + done * n, ze, cnt * n * sizeof(Fr));
            DEV_TRY(hipStreamSynchronize(pc->st));  // the next slice rewrites the plan
        }
    });
}

extern "C" int kzgamd_poly_recover(void* vpc, blst_fr* out, const blst_fr* samples, const uint8_t* present, size_t n, size_t nprob,
                                   int coeffs) {
    PolyCtx* pc = (PolyCtx*)vpc;
    if (!pc) return -1;
    if (!is_pow2(n)) return 1;
    if (nprob == 0) return 0;
    if (!out || !samples || !present) return -1;
    std::vector<u64> missing;
    std::vector<size_t> offsets;
    size_t maxcount = 0;
    try {
        offsets.assign(nprob + 1, 0);
        for (size_t b = 0; b < nprob; ++b) {
            for (size_t i = 0; i < n; ++i)
                if (!present[b * n + i]) missing.push_back(i);
            offsets[b + 1] = missing.size();
            const size_t cnt = offsets[b + 1] - offsets[b];
            if (cnt > n / 2) return 2;
            if (cnt > maxcount) maxcount = cnt;
        }
    } catch (...) {
        return -2;  // no host memory for the index lists
    }
    const size_t W = pc->ntt->W;
    if (n > W) return 3;
    const bool direct = maxcount <= ZP_DIRECT_MAX;
    const Fr five = fr_small(5), fifth = ff::inverse_bgcd(five);
    ZeroPlan pl;
    return run_call(pc, [&] {
        const size_t per = slice_of(pc, nprob, (12 * n + maxcount) * sizeof(Fr) + maxcount * sizeof(u64) + n);
        pc->a.ensure(per * n * sizeof(Fr));
        pc->b.ensure(per * n * sizeof(Fr));
        pc->c.ensure(per * n * sizeof(Fr));
        pc->out.ensure(per * n * sizeof(Fr));
        pc->mask.ensure(per * n);
        hipStream_t st = pc->st;
        for (size_t done = 0; done < nprob; done += per) {
            const size_t cnt = min_sz(per, nprob - done), tot = cnt * n;
            zero_plan_build(pl, cnt, [&](size_t b) { return offsets[done + b + 1] - offsets[done + b]; });
            zero_reserve(pc, pl, direct, 2 * tot);
            Fr *a = pc->a.as<Fr>(), *zp = pc->b.as<Fr>(), *ze = pc->c.as<Fr>(), *o = pc->out.as<Fr>();
            Fr *f = pc->f.as<Fr>(), *g = pc->g.as<Fr>();
            upload(pc, a, samples + done * n, tot * sizeof(Fr));
            upload(pc, pc->mask.p, present + done * n, tot);
            enqueue_zero(pc, zp, ze, n, W / n, pl, missing.data() + offsets[done], direct, true);
            hipLaunchKernelGGL(k_rc_mask, dim3(blocks(tot)), dim3(256), 0, st, o, (const Fr*)a, pc->mask.as<uint8_t>(), (const Fr*)ze, tot);
            zntt(pc, a, o, n, cnt, 1);
            hipLaunchKernelGGL(k_rc_shift, dim3(blocks(2 * tot)), dim3(256), 0, st, f, (const Fr*)a, (const Fr*)zp, fifth, n, 2 * tot);
            zntt(pc, g, f, n, 2 * cnt, 0);
            hipLaunchKernelGGL(k_rc_div, dim3(blocks(tot)), dim3(256), 0, st, o, (const Fr*)g, n, tot);
            zntt(pc, a, o, n, cnt, 1);
            hipLaunchKernelGGL(k_rc_scale, dim3(blocks(tot)), dim3(256), 0, st, a, five, n, tot);
            DEV_TRY(hipGetLastError());
            if (coeffs) {
                download(pc, out + done * n, a, tot * sizeof(Fr));
            } else {
                zntt(pc, o, a, n, cnt, 0);
                download(pc, out + done * n, o, tot * sizeof(Fr));
            }
            DEV_TRY(hipStreamSynchronize(st));  // the next slice rewrites the plan
        }
    });
}
