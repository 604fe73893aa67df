// A prepared bucket MSM in G2:
//     out[b] = sum_{i < n} scalars[b * n + i] * points[i]     kzgamd_g2_msm on the handle of kzgamd_g2_msm_new
//
// The handle keeps T[k][i] = 2^(8k) * points[i] as affine points, k < 32 windows.  A call recodes every scalar into 32
// signed base-256 digits (g2_bucket.hip.h, the recoding of groupmul.hip); every non-zero digit d of scalar i in window k
// is one ENTRY: the table index k * npoints + i with a sign bit, in bucket |d| (1 .. 128) of its batch item.  The
// entries are grouped by (batch item, bucket) with a counting sort over a count matrix [key][workgroup] and its scan (no
// global atomic in a call: the one of this file marks an infinite table entry at creation), a bucket's entries are cut into segments that a lane each adds up from the table, the
// partial sums of a bucket (contiguous) are summed by further levels of the same shape until one is left, and
//     out[b] = sum_{j = 1 .. 128} j * B[b][j]
// by a lane per bucket (7 doublings, at most 7 additions) and the one-wave LDS tree over the 128.  No doubling per
// point: at most 32 mixed additions.  Calls above the pass cap run in passes, whose results are added.
//
// Every addition is a complete one (g2::madd_tab, g2::add): callers repeat points, so equal points in a bucket are
// ordinary, P and -P meet, and points outside the subgroup have infinite table entries.  Workgroups are one wave,
// ordered by fpw::wave_sync; nothing waits on data, and every loop is bounded by a count fixed at launch.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <string>

#include "../../include/kzg_mi355x.h"
#include "config.h"
#include "device_guard.h"
#include "ff.hip.h"
#include "fpw.hip.h"
#include "g2_28.hip.h"
#include "g2_bucket.hip.h"
#include "host_call.h"

using ff::Fr;
using ff::u32;
using kzgamd::blocks;
using kzgamd::DevArray;

namespace {

constexpr int LANES = 64;
constexpr int NWIN = g2b::NWIN;
constexpr int NBUCKET = g2b::HALF;                       // buckets of a batch item
constexpr size_t SEGMENT_DEFAULT = 8;                    // entries a lane accumulates: of 8 .. 64 the fastest at 2^15 points, level with 16 at 2^20 (profiles/g2_msm_time.jsonl)
constexpr size_t PASS_DEFAULT = (size_t)1 << 25;         // entries per pass: 2^20 points of one batch item
constexpr size_t PASS_MAX = (size_t)1 << 30;             // offsets are 32-bit
constexpr size_t POINTS_MAX = (size_t)1 << 26;           // 32 * npoints and the sign bit fit an entry
constexpr size_t TAB_CHUNK = (size_t)1 << 16;            // points per launch of the table kernels (a wave on every SIMD): 705 MB of columns
constexpr u32 SCAN_PER_LANE = 16, SCAN_BLOCK = LANES * SCAN_PER_LANE;
constexpr unsigned GRID_Y_MAX = 32768;
static_assert(NBUCKET == 2 * LANES, "a lane counts, places and sums two buckets");

// ---------------------------------------------------------------- the table
// lane i < cnt: col[k * cnt + i] = 2^(8k) * points[i], k < 32; an infinite point gives an infinite column
__global__ void __launch_bounds__(LANES) k_g2msm_columns(g2::Jac* __restrict__ col, const ff::Fp* __restrict__ points, size_t cnt) {
    const size_t i = (size_t)blockIdx.x * LANES + threadIdx.x;
    if (i >= cnt) return;
    g2::Jac p;
    g2::from_blst_jacobian(p, points + 6 * i);
#pragma unroll 1
    for (int k = 0; k < NWIN; ++k) {
        col[(size_t)k * cnt + i] = p;
        if (k + 1 < NWIN) g2b::next_window(p);
    }
}
// lane t < 32 * cnt: the column entry to affine form at its place in the table; an infinite one sets its bit
__global__ void __launch_bounds__(LANES) k_g2msm_affine(g2::AffPt* __restrict__ tab, u32* __restrict__ inf_mask,
                                                        const g2::Jac* __restrict__ col, size_t at, size_t cnt, size_t npoints) {
    const size_t t = (size_t)blockIdx.x * LANES + threadIdx.x;
    if (t >= (size_t)NWIN * cnt) return;
    const size_t k = t / cnt, i = t % cnt;
    g2::AffPt a;
    g2::to_affine(a, col[t]);
    tab[k * npoints + at + i] = a;
    if (a.flags & 1) atomicOr(&inf_mask[at + i], 1u << k);
}

// ---------------------------------------------------------------- grouping
// One pass: batch items b0 .. b0 + gridDim.y - 1, points i0 .. i1 - 1 of each; a workgroup has 64 points of one item.
struct Pass {
    const Fr* sc;         // all scalars of the call
    const u32* inf_mask;  // per point: the windows whose table entry is infinite
    size_t n, b0, i0, i1;
    u32 npoints, nblk;    // points per window of the table; workgroups per batch item
};

// cnt[(by * 128 + j) * nblk + blk] = entries of workgroup (blk, by) in bucket j + 1
__global__ void __launch_bounds__(LANES) k_g2msm_count(u32* __restrict__ cnt, Pass ps) {
    __shared__ u32 h[NBUCKET];
    const int t = threadIdx.x;
    h[t] = h[t + LANES] = 0;
    fpw::wave_sync();
    const size_t i = ps.i0 + (size_t)blockIdx.x * LANES + t;
    if (i < ps.i1) {
        const Fr k = ff::from_mont(ps.sc[(ps.b0 + blockIdx.y) * ps.n + i]);
        g2b::for_each_entry(k, (u32)i, ps.npoints, ps.inf_mask[i], [&](u32 bucket, u32) { atomicAdd(&h[bucket - 1], 1u); });
    }
    fpw::wave_sync();
    for (int j = t; j < NBUCKET; j += LANES) cnt[((size_t)blockIdx.y * NBUCKET + j) * ps.nblk + blockIdx.x] = h[j];
}
// the entries to their places: off is the scanned count matrix
__global__ void __launch_bounds__(LANES) k_g2msm_scatter(u32* __restrict__ entries, const u32* __restrict__ off, Pass ps) {
    __shared__ u32 at[NBUCKET];
    const int t = threadIdx.x;
    for (int j = t; j < NBUCKET; j += LANES) at[j] = off[((size_t)blockIdx.y * NBUCKET + j) * ps.nblk + blockIdx.x];
    fpw::wave_sync();
    const size_t i = ps.i0 + (size_t)blockIdx.x * LANES + t;
    if (i < ps.i1) {
        const Fr k = ff::from_mont(ps.sc[(ps.b0 + blockIdx.y) * ps.n + i]);
        g2b::for_each_entry(k, (u32)i, ps.npoints, ps.inf_mask[i], [&](u32 bucket, u32 value) { entries[atomicAdd(&at[bucket - 1], 1u)] = value; });
    }
}

// ---------------------------------------------------------------- an exclusive scan of m 32-bit counts, in place
__device__ __forceinline__ u32 wave_inclusive(u32 v, int t) {
#pragma unroll
    for (int d = 1; d < LANES; d <<= 1) {
        const u32 o = __shfl_up(v, d, LANES);
        if (t >= d) v += o;
    }
    return v;
}
// a workgroup scans its 1024 counts and leaves their sum in bsum[block]
__global__ void __launch_bounds__(LANES) k_g2msm_scan_local(u32* __restrict__ d, u32* __restrict__ bsum, size_t m) {
    const int t = threadIdx.x;
    const size_t base = ((size_t)blockIdx.x * LANES + t) * SCAN_PER_LANE;
    u32 sum = 0;
    for (u32 k = 0; k < SCAN_PER_LANE; ++k)
        if (base + k < m) sum += d[base + k];
    const u32 incl = wave_inclusive(sum, t);
    u32 run = incl - sum;
    for (u32 k = 0; k < SCAN_PER_LANE; ++k)
        if (base + k < m) {
            const u32 v = d[base + k];
            d[base + k] = run;
            run += v;
        }
    if (t == LANES - 1) bsum[blockIdx.x] = incl;
}
// one wave scans the nb workgroup sums
__global__ void __launch_bounds__(LANES) k_g2msm_scan_top(u32* __restrict__ bsum, size_t nb) {
    const int t = threadIdx.x;
    u32 carry = 0;
    for (size_t at = 0; at < nb; at += LANES) {
        const u32 v = at + t < nb ? bsum[at + t] : 0;
        const u32 incl = wave_inclusive(v, t);
        if (at + t < nb) bsum[at + t] = carry + incl - v;
        carry += __shfl(incl, LANES - 1, LANES);
    }
}
__global__ void __launch_bounds__(256) k_g2msm_scan_add(u32* __restrict__ d, const u32* __restrict__ bsum, size_t m) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) d[i] += bsum[i / SCAN_BLOCK];
}

// ---------------------------------------------------------------- levels
// ko[key] = where the entries of key begin, key <= K (ko[K]: their count)
__global__ void __launch_bounds__(256) k_g2msm_key_offsets(u32* __restrict__ ko, const u32* __restrict__ off, u32 nblk, size_t K) {
    const size_t key = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (key <= K) ko[key] = off[key * nblk];
}
// ns[key] = segments of the key's items, ns[K] = 0: scanned in place, it is the next level's offsets
__global__ void __launch_bounds__(256) k_g2msm_segments(u32* __restrict__ ns, const u32* __restrict__ in_off, u32 seg, size_t K) {
    const size_t key = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (key < K) ns[key] = g2b::segments(in_off[key + 1] - in_off[key], seg);
    else if (key == K) ns[key] = 0;
}
// lane s < out_off[K]: partial sum s = the sum of its segment of table entries
__global__ void __launch_bounds__(LANES) k_g2msm_accum(g2::Jac* __restrict__ out, const g2::AffPt* __restrict__ tab,
                                                       const u32* __restrict__ entries, const u32* __restrict__ in_off,
                                                       const u32* __restrict__ out_off, u32 seg, u32 K) {
    const size_t s = (size_t)blockIdx.x * LANES + threadIdx.x;
    if (s >= out_off[K]) return;
    const u32 key = g2b::key_of(out_off, K, (u32)s);
    u32 lo, hi;
    g2b::segment_range(in_off[key + 1] - in_off[key], seg, (u32)s - out_off[key], lo, hi);
    g2::Jac acc;
    g2b::chain_entries(acc, tab, entries + in_off[key] + lo, hi - lo);
    out[s] = acc;
}
// the same over the partial sums of the level before
__global__ void __launch_bounds__(LANES) k_g2msm_level(g2::Jac* __restrict__ out, const g2::Jac* __restrict__ in,
                                                       const u32* __restrict__ in_off, const u32* __restrict__ out_off, u32 seg, u32 K) {
    const size_t s = (size_t)blockIdx.x * LANES + threadIdx.x;
    if (s >= out_off[K]) return;
    const u32 key = g2b::key_of(out_off, K, (u32)s);
    u32 lo, hi;
    g2b::segment_range(in_off[key + 1] - in_off[key], seg, (u32)s - out_off[key], lo, hi);
    g2::Jac acc;
    g2b::chain_partials(acc, in + in_off[key] + lo, hi - lo);
    out[s] = acc;
}

// ---------------------------------------------------------------- reduction
// w[key] = (bucket index of key) * (the one partial sum of key, or infinity for an empty bucket)
__global__ void __launch_bounds__(LANES) k_g2msm_weigh(g2::Jac* __restrict__ w, const g2::Jac* __restrict__ part, const u32* __restrict__ off, u32 K) {
    const size_t key = (size_t)blockIdx.x * LANES + threadIdx.x;
    if (key >= K) return;
    g2::Jac r;
    if (off[key + 1] != off[key]) g2b::weigh(r, part[off[key]], (u32)(key % NBUCKET) + 1);  // the sum stays in memory: no copy in registers
    else g2::set_inf(r);
    w[key] = r;
}
// acc[b0 + block] += the sum of the block's 128 weighted bucket sums: the one-wave LDS tree of setupcheck.hip
__global__ void __launch_bounds__(LANES) k_g2msm_reduce(g2::Jac* __restrict__ acc, const g2::Jac* __restrict__ w, size_t b0) {
    __shared__ g2::Jac slots[LANES];
    const int t = threadIdx.x;
    const g2::Jac* mine = w + (size_t)blockIdx.x * NBUCKET;
    slots[t] = mine[t];
    fpw::wave_sync();
#pragma unroll 1
    for (int half = LANES; half >= 1; half >>= 1) {  // the first level takes its other operand from memory
        if (t < half) {
            g2::Jac a = slots[t];
            g2::add(a, half == LANES ? mine[t + LANES] : slots[t + half]);
            slots[t] = a;
        }
        fpw::wave_sync();
    }
    if (t == 0) {
        g2::Jac r = slots[0];
        g2::add(r, acc[b0 + blockIdx.x]);
        acc[b0 + blockIdx.x] = r;
    }
}
// out[b] = acc[b] in the blst_p2 layout with Z = one (canonical; infinity all-zero)
__global__ void __launch_bounds__(LANES) k_g2msm_out(ff::Fp* __restrict__ out, const g2::Jac* __restrict__ acc, size_t nbatch) {
    const size_t b = (size_t)blockIdx.x * LANES + threadIdx.x;
    if (b >= nbatch) return;
    g2::AffPt a;
    g2::to_affine(a, acc[b]);
    g2::Jac p;
    if (a.flags & 1) g2::set_inf(p);
    else g2::set_affine(p, a.x, a.y);
    g2::to_blst_jacobian(out + 6 * b, p);
}

// ---------------------------------------------------------------- host side
struct G2MsmCtx {
    int device = 0;
    std::mutex mu;
    hipStream_t st = nullptr;
    size_t npoints = 0, segment = SEGMENT_DEFAULT, pass_entries = PASS_DEFAULT;
    DevArray<g2::AffPt> tab;   // T[k * npoints + i]
    DevArray<u32> inf_mask;    // per point
    // workspace of a call, grown as calls need it
    DevArray<Fr> sc;
    DevArray<u32> cnt, bsum, entries, ko, offa, offb;
    DevArray<g2::Jac> parta, partb, weighed, acc;
    DevArray<blst_p2> res;
    ~G2MsmCtx() {
        if (st) (void)hipStreamDestroy(st);
    }
};

// d[0 .. m) becomes its exclusive prefix sums
void enqueue_scan(G2MsmCtx* c, u32* d, size_t m) {
    const size_t nb = (m + SCAN_BLOCK - 1) / SCAN_BLOCK;
    c->bsum.ensure(nb);
    hipLaunchKernelGGL(k_g2msm_scan_local, dim3((unsigned)nb), dim3(LANES), 0, c->st, d, c->bsum.p, m);
    if (nb == 1) return;
    hipLaunchKernelGGL(k_g2msm_scan_top, dim3(1), dim3(LANES), 0, c->st, c->bsum.p, nb);
    hipLaunchKernelGGL(k_g2msm_scan_add, dim3(blocks(m)), dim3(256), 0, c->st, d, (const u32*)c->bsum.p, m);
}

// one pass: acc[b0 + by] += sum over the points i0 .. i1 - 1 of batch item b0 + by, by < nb
void enqueue_pass(G2MsmCtx* c, size_t n, size_t b0, size_t nb, size_t i0, size_t i1) {
    hipStream_t st = c->st;
    const size_t npts = i1 - i0, nblk = blocks(npts, LANES), K = nb * NBUCKET, m = K * nblk + 1;
    const size_t emax = nb * npts * NWIN;  // entries
    const u32 seg = (u32)c->segment;
    Pass ps{c->sc.p, c->inf_mask.p, n, b0, i0, i1, (u32)c->npoints, (u32)nblk};
    c->cnt.ensure(m);
    c->entries.ensure(emax);
    c->ko.ensure(K + 1);
    c->offa.ensure(K + 1);
    c->offb.ensure(K + 1);
    const size_t s0max = emax / seg + K;  // partial sums of the first level, at most
    c->parta.ensure(s0max);
    c->partb.ensure(s0max / seg + K);
    c->weighed.ensure(K);

    const dim3 grid((unsigned)nblk, (unsigned)nb);
    hipLaunchKernelGGL(k_g2msm_count, grid, dim3(LANES), 0, st, c->cnt.p, ps);
    DEV_TRY(hipMemsetAsync(c->cnt.p + (m - 1), 0, sizeof(u32), st));
    enqueue_scan(c, c->cnt.p, m);
    hipLaunchKernelGGL(k_g2msm_scatter, grid, dim3(LANES), 0, st, c->entries.p, (const u32*)c->cnt.p, ps);
    hipLaunchKernelGGL(k_g2msm_key_offsets, dim3(blocks(K + 1)), dim3(256), 0, st, c->ko.p, (const u32*)c->cnt.p, (u32)nblk, K);

    // the levels: a bucket holds at most every entry of its batch item
    const u32* in_off = c->ko.p;
    u32 *out_off = c->offa.p, *spare = c->offb.p;
    g2::Jac *out = c->parta.p, *in = c->partb.p;
    size_t most = npts * NWIN, rest = emax / seg, lanes = s0max;  // the largest bucket and the items of the level, at most
    for (int level = 0;; ++level) {
        hipLaunchKernelGGL(k_g2msm_segments, dim3(blocks(K + 1)), dim3(256), 0, st, out_off, in_off, seg, K);
        enqueue_scan(c, out_off, K + 1);
        if (level == 0)
            hipLaunchKernelGGL(k_g2msm_accum, dim3(blocks(lanes, LANES)), dim3(LANES), 0, st, out, (const g2::AffPt*)c->tab.p,
                               (const u32*)c->entries.p, in_off, (const u32*)out_off, seg, (u32)K);
        else
            hipLaunchKernelGGL(k_g2msm_level, dim3(blocks(lanes, LANES)), dim3(LANES), 0, st, out, (const g2::Jac*)in, in_off,
                               (const u32*)out_off, seg, (u32)K);
        most = (most + seg - 1) / seg;
        if (most <= 1) break;
        rest /= seg;
        lanes = rest + K;  // sum of ceil(c / seg^(level + 2)) over the K keys
        g2::Jac* tp = in;
        in = out;
        out = tp;
        u32* to = level == 0 ? spare : const_cast<u32*>(in_off);
        in_off = out_off;
        out_off = to;
    }
    hipLaunchKernelGGL(k_g2msm_weigh, dim3(blocks(K, LANES)), dim3(LANES), 0, st, c->weighed.p, (const g2::Jac*)out, (const u32*)out_off, (u32)K);
    hipLaunchKernelGGL(k_g2msm_reduce, dim3((unsigned)nb), dim3(LANES), 0, st, c->acc.p, (const g2::Jac*)c->weighed.p, b0);
    DEV_TRY(hipGetLastError());
}

// the table of `points`, chunk by chunk through one buffer of columns; complete when this returns
void build_table(G2MsmCtx* c, const blst_p2* points) {
    const size_t np = c->npoints, chunk = np < TAB_CHUNK ? np : TAB_CHUNK;
    c->tab.ensure((size_t)NWIN * np);
    c->inf_mask.ensure(np);
    DEV_TRY(hipMemsetAsync(c->inf_mask.p, 0, np * sizeof(u32), c->st));
    DevArray<blst_p2> pts;
    DevArray<g2::Jac> col;
    pts.ensure(chunk);
    col.ensure((size_t)NWIN * chunk);
    for (size_t at = 0; at < np; at += chunk) {
        const size_t cnt = np - at < chunk ? np - at : chunk;
        DEV_TRY(hipMemcpyAsync(pts.p, points + at, cnt * sizeof(blst_p2), hipMemcpyHostToDevice, c->st));
        hipLaunchKernelGGL(k_g2msm_columns, dim3(blocks(cnt, LANES)), dim3(LANES), 0, c->st, col.p, (const ff::Fp*)pts.p, cnt);
        hipLaunchKernelGGL(k_g2msm_affine, dim3(blocks((size_t)NWIN * cnt, LANES)), dim3(LANES), 0, c->st, c->tab.p, c->inf_mask.p,
                           (const g2::Jac*)col.p, at, cnt, np);
        DEV_TRY(hipGetLastError());
    }
    DEV_TRY(hipStreamSynchronize(c->st));
}

size_t table_bytes_of(size_t npoints) { return npoints * NWIN * sizeof(g2::AffPt); }
// what build_table allocates: the table, the mask, and one chunk of points and of columns
size_t creation_bytes_of(size_t npoints) {
    const size_t chunk = npoints < TAB_CHUNK ? npoints : TAB_CHUNK;
    return table_bytes_of(npoints) + npoints * sizeof(u32) + chunk * (NWIN * sizeof(g2::Jac) + sizeof(blst_p2));
}

}  // namespace

extern "C" void* kzgamd_g2_msm_new(const blst_p2* points, size_t npoints, const KzgAmdConfig* cfg, int* err) {
    int dummy;
    if (!err) err = &dummy;
    *err = 0;
    if (npoints && !points) {
        *err = -1;
        return nullptr;
    }
    int device = -1;
    long long seg = (long long)SEGMENT_DEFAULT, pass = (long long)PASS_DEFAULT;
    uint64_t budget = 0;
    if (cfg) {
        bool ok = cfg->struct_size >= offsetof(KzgAmdConfig, tuning) + sizeof(cfg->tuning);
        if (ok && cfg->tuning) {
            std::string rest, none;
            ok = kzgamd::take_key(cfg->tuning, "g2msm_segment", 2, 1 << 20, &seg, &rest) &&
                 kzgamd::take_key(rest.c_str(), "g2msm_pass_entries", 32, (long long)PASS_MAX, &pass, &none) && none.empty() &&
                 !(seg & (seg - 1)) && pass % 32 == 0;
        }
        if (!ok) {
            fprintf(stderr, "kzg_mi355x: kzgamd_g2_msm_new: a malformed KzgAmdConfig, or tuning: the keys of this handle are "
                            "'g2msm_segment' (a power of two, at least 2) and 'g2msm_pass_entries' (a multiple of 32, at least 32)\n");
            *err = -2;
            return nullptr;
        }
        device = cfg->device;
        budget = cfg->table_budget_bytes;
    }
    if (npoints > POINTS_MAX || (budget && table_bytes_of(npoints) > budget)) {
        *err = 2;
        return nullptr;
    }
    if (device < 0) {
        const hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess) {
            *err = kzgamd::dev_code(e);
            return nullptr;
        }
    }
    if (npoints) {  // the table and the workspace of its creation against the memory that is free on the device
        *err = kzgamd::status_of([&]() -> int {
            kzgamd::DeviceGuard on_device(device);
            DEV_TRY(on_device.err);
            size_t free_b = 0, total_b = 0;
            DEV_TRY(hipMemGetInfo(&free_b, &total_b));
            return creation_bytes_of(npoints) > free_b ? 2 : 0;
        });
        if (*err) return nullptr;
    }
    return kzgamd::create_handle<G2MsmCtx>(device, err, [&](G2MsmCtx* c) {
        c->npoints = npoints;
        c->segment = (size_t)seg;
        c->pass_entries = (size_t)pass;
        DEV_TRY(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
        if (npoints) build_table(c, points);
    });
}

extern "C" void kzgamd_g2_msm_free(void* h) {
    G2MsmCtx* c = (G2MsmCtx*)h;
    if (!c) return;
    kzgamd::DeviceGuard on_device(c->device);
    delete c;
}

extern "C" int kzgamd_g2_msm_info(void* h, size_t* npoints, int* window_bits, size_t* segment, size_t* pass_entries, size_t* table_bytes) {
    G2MsmCtx* c = (G2MsmCtx*)h;
    if (!c) return -1;
    if (npoints) *npoints = c->npoints;
    if (window_bits) *window_bits = g2b::WBITS;
    if (segment) *segment = c->segment;
    if (pass_entries) *pass_entries = c->pass_entries;
    if (table_bytes) *table_bytes = table_bytes_of(c->npoints);
    return 0;
}

extern "C" int kzgamd_g2_msm(void* h, blst_p2* out, const blst_fr* scalars, size_t n, size_t nbatch) {
    G2MsmCtx* c = (G2MsmCtx*)h;
    if (!c) return -1;
    if (nbatch == 0) return 0;
    if (!out || (n && !scalars)) return -1;
    if (n > c->npoints) return 1;
    if (n == 0) {
        memset(out, 0, nbatch * sizeof(blst_p2));
        return 0;
    }
    return kzgamd::run_call(c, [&] {
        hipStream_t st = c->st;
        c->sc.ensure(nbatch * n);
        c->acc.ensure(nbatch);
        c->res.ensure(nbatch);
        DEV_TRY(hipMemcpyAsync(c->sc.p, scalars, nbatch * n * sizeof(Fr), hipMemcpyHostToDevice, st));
        DEV_TRY(hipMemsetAsync(c->acc.p, 0, nbatch * sizeof(g2::Jac), st));  // infinity: Z all-zero
        const size_t per_item = n * NWIN;
        if (per_item <= c->pass_entries) {  // whole batch items per pass
            size_t per = c->pass_entries / per_item;
            if (per > GRID_Y_MAX) per = GRID_Y_MAX;
            for (size_t b0 = 0; b0 < nbatch; b0 += per) enqueue_pass(c, n, b0, nbatch - b0 < per ? nbatch - b0 : per, 0, n);
        } else {  // a range of points of one batch item per pass
            const size_t pts = c->pass_entries / NWIN;
            for (size_t b = 0; b < nbatch; ++b)
                for (size_t i0 = 0; i0 < n; i0 += pts) enqueue_pass(c, n, b, 1, i0, n - i0 < pts ? n : i0 + pts);
        }
        hipLaunchKernelGGL(k_g2msm_out, dim3(blocks(nbatch, LANES)), dim3(LANES), 0, st, (ff::Fp*)c->res.p, (const g2::Jac*)c->acc.p, nbatch);
        DEV_TRY(hipGetLastError());
        DEV_TRY(hipMemcpyAsync(out, c->res.p, nbatch * sizeof(blst_p2), hipMemcpyDeviceToHost, st));
    });
}
