// G2 linear combinations on the GPU, and the verification of a trusted setup built from them:
//     *out = sum_i scalars[i] * points[i]     kzgamd_g2_lincomb
//     is this (M, L, Q) a setup at all?       kzgamd_verify_trusted_setup / kzgamd_verify_trusted_setup_file
//
// The linear combination: a lane per point in one-wave workgroups (g2lc::term: the point to affine form with an
// inversion of its own, then a left-to-right double-and-add over the 256 bits of the scalar), the 64 terms of a
// workgroup summed pairwise through LDS with g2::add, and the sums of the workgroups by further launches of k_g2_sum (64
// operands per workgroup) until one is left.  Every loop is bounded by a constant or by the count; nothing waits on data.
// Counts above the slice run slice by slice through one workspace, and the slice sums are summed the same way.
//
// The verification: a challenge r from a seed (the caller's, or a hash of the whole setup), its powers
// on the device, and four checks: the generators, e(B, Q[0]) == e(A, Q[1]) and e(M[1], C) == e(M[0], D) over
// r-combinations of consecutive points (A, B: rows of one batched G1 MSM over M; C, D: two runs of the G2 linear
// combination over Q), and sum_i f[i] L[i] == sum_k r^k M[k] with f the forward transform of the powers.  The G1 side
// is composed from what msm.hip, ntt.hip and codec.hip export; the two pairing checks run on the host.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/kzg_mi355x.h"
#include "config.h"
#include "device_guard.h"
#include "ff.hip.h"
#include "fpw.hip.h"
#include "g2_28.hip.h"
#include "g2_lincomb.hip.h"
#include "host_call.h"
#include "host_fp64.h"
#include "host_g1.h"
#include "host_pairing.h"
#include "msm_internal.h"
#include "ntt_internal.h"
#include "setupcheck_internal.h"
#include "sha256.h"

using ff::Fr;
using kzgamd::blocks;
using kzgamd::ScopedBuf;

namespace {

constexpr int LANES = g2lc::LANES;
constexpr size_t SLICE_DEFAULT = (size_t)1 << 18;  // points per slice: 75 MB of blst_p2, 8 MB of scalars
constexpr size_t SLICE_MIN = 64;

// the 64 points the lanes of a one-wave workgroup hold, summed into slot 0.  The workgroup IS one wave, so the levels
// are ordered by fpw::wave_sync (LDS accesses of a wave in program order), not by a workgroup barrier.
static_assert(LANES == 64, "tree_sum: a workgroup is one wave");
__device__ __forceinline__ void tree_sum(g2::Jac* slots, const g2::Jac& mine, int t) {
    slots[t] = mine;
    fpw::wave_sync();
#pragma unroll 1
    for (int half = LANES / 2; half >= 1; half >>= 1) {
        if (t < half) g2lc::tree_step(slots, t, half);
        fpw::wave_sync();
    }
}

// part[block] = sum of scalars[i] * points[i] over the block's 64 indices below n
__global__ void __launch_bounds__(LANES) k_g2_lincomb_terms(g2::Jac* __restrict__ part, const ff::Fp* __restrict__ points,
                                                            const Fr* __restrict__ scalars, size_t n) {
    __shared__ g2::Jac slots[LANES];
    const int t = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * LANES + t;
    g2::Jac acc;
    g2::set_inf(acc);
    if (i < n) g2lc::term(acc, points + 6 * i, scalars[i]);
    tree_sum(slots, acc, t);
    if (t == 0) part[blockIdx.x] = slots[0];
}

// out[block] = sum of the block's 64 points of in[0 .. n)
__global__ void __launch_bounds__(LANES) k_g2_sum(g2::Jac* __restrict__ out, const g2::Jac* __restrict__ in, size_t n) {
    __shared__ g2::Jac slots[LANES];
    const int t = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * LANES + t;
    g2::Jac acc;
    g2::set_inf(acc);
    if (i < n) acc = in[i];
    tree_sum(slots, acc, t);
    if (t == 0) out[blockIdx.x] = slots[0];
}

// one point to the blst_p2 layout (canonical; infinity all-zero)
__global__ void __launch_bounds__(LANES) k_g2_out(ff::Fp* __restrict__ out, const g2::Jac* __restrict__ in) {
    if (blockIdx.x == 0 && threadIdx.x == 0) g2::to_blst_jacobian(out, *in);
}

// *dst = the sum of the m >= 1 points of `a`; a and b (room for blocks(m, 64) points) are both clobbered.
// At most 6 launches: m shrinks 64-fold with each.
void enqueue_sum(g2::Jac* dst, g2::Jac* a, g2::Jac* b, size_t m, hipStream_t st) {
    for (;;) {
        const size_t nb = blocks(m, LANES);
        hipLaunchKernelGGL(k_g2_sum, dim3((unsigned)nb), dim3(LANES), 0, st, nb == 1 ? dst : b, (const g2::Jac*)a, m);
        if (nb == 1) return;
        g2::Jac* t = a;
        a = b;
        b = t;
        m = nb;
    }
}

// the two buffers of a run over up to n points, and the slot its sum lands in
struct Work {
    g2::Jac *a, *b, *sum;
    size_t na, nb;
    Work(void* p, size_t n) {
        na = blocks(n, LANES);
        nb = blocks(na, LANES);
        a = (g2::Jac*)p;
        b = a + na;
        sum = b + nb;
    }
    static size_t bytes(size_t n) {
        const size_t na = blocks(n, LANES);
        return (na + blocks(na, LANES) + 1) * sizeof(g2::Jac);
    }
};

// *dst = sum_i scalars[i] * points[i], i < n, n >= 1
void enqueue_lincomb(g2::Jac* dst, const void* d_points, const void* d_scalars, size_t n, const Work& w, hipStream_t st) {
    hipLaunchKernelGGL(k_g2_lincomb_terms, dim3((unsigned)blocks(n, LANES)), dim3(LANES), 0, st, w.a, (const ff::Fp*)d_points,
                       (const Fr*)d_scalars, n);
    enqueue_sum(dst, w.a, w.b, blocks(n, LANES), st);
}

}  // namespace

size_t kzgamd::g2lc_gpu::work_bytes(size_t n) { return Work::bytes(n); }

void kzgamd::g2lc_gpu::lincomb_enqueue(void* d_out, const void* d_points, const void* d_scalars, size_t n, void* d_work,
                                       hipStream_t st) {
    const Work w(d_work, n);
    enqueue_lincomb(w.sum, d_points, d_scalars, n, w, st);
    hipLaunchKernelGGL(k_g2_out, dim3(1), dim3(LANES), 0, st, (ff::Fp*)d_out, (const g2::Jac*)w.sum);
}

extern "C" int kzgamd_g2_lincomb_info(size_t* slice_points) {
    if (slice_points) *slice_points = SLICE_DEFAULT;
    return 0;
}

extern "C" int kzgamd_g2_lincomb(blst_p2* out, const blst_p2* points, const blst_fr* scalars, size_t n, const KzgAmdConfig* cfg) {
    if (!out) return -1;
    if (n && (!points || !scalars)) return -1;
    int device;
    size_t slice;
    if (int rc = kzgamd::read_slice_config(cfg, "kzgamd_g2_lincomb", "lincomb_slice", SLICE_DEFAULT, SLICE_MIN, &device, &slice)) return rc;
    if (n == 0) {
        memset(out, 0, sizeof *out);
        return 0;
    }
    return kzgamd::status_of([&] {
        if (device < 0) DEV_TRY(hipGetDevice(&device));
        kzgamd::DeviceGuard on_device(device);
        DEV_TRY(on_device.err);
        kzgamd::CallStream s;
        if (slice > n) slice = n;
        const size_t nslices = (n + slice - 1) / slice;
        ScopedBuf pts, sc, work, sums, res;
        pts.alloc(slice * sizeof(blst_p2));
        sc.alloc(slice * sizeof(Fr));
        work.alloc(Work::bytes(slice));
        sums.alloc(Work::bytes(nslices * LANES));  // a: the slice sums (nslices <= blocks(nslices * 64, 64)), b, the total
        res.alloc(sizeof(blst_p2));
        const Work w(work.p, slice), total(sums.p, nslices * LANES);
        for (size_t at = 0, k = 0; at < n; at += slice, ++k) {
            const size_t cnt = n - at < slice ? n - at : slice;
            DEV_TRY(hipMemcpyAsync(pts.p, points + at, cnt * sizeof(blst_p2), hipMemcpyHostToDevice, s.st));
            DEV_TRY(hipMemcpyAsync(sc.p, scalars + at, cnt * sizeof(Fr), hipMemcpyHostToDevice, s.st));
            enqueue_lincomb(total.a + k, pts.p, sc.p, cnt, w, s.st);
            DEV_TRY(hipGetLastError());
            DEV_TRY(hipStreamSynchronize(s.st));  // the next slice overwrites what this one reads
        }
        enqueue_sum(total.sum, total.a, total.b, nslices, s.st);
        hipLaunchKernelGGL(k_g2_out, dim3(1), dim3(LANES), 0, s.st, (ff::Fp*)res.p, (const g2::Jac*)total.sum);
        DEV_TRY(hipGetLastError());
        DEV_TRY(hipMemcpyAsync(out, res.p, sizeof(blst_p2), hipMemcpyDeviceToHost, s.st));
        DEV_TRY(hipStreamSynchronize(s.st));
    });
}

// ---------------------------------------------------------------- the verification of a trusted setup
namespace {

namespace hp = kzgamd::pairing;

const char SEED_DOMAIN[] = "KZGAMD_VERIFY_SETUP_V1";  // 22 bytes, no terminator hashed

// hash_to_bls_field: the 32 bytes as a big-endian integer mod r, Montgomery form (as `secret` of the generator)
Fr hash_to_bls_field(const uint8_t b[32]) {
    Fr s;
    for (int i = 0; i < 8; ++i) {
        const uint8_t* q = b + (7 - i) * 4;
        s.v[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
    }
    return ff::mul(s, Fr::r2());
}

void put_be64(kzgamd::Sha256& h, uint64_t v) {
    uint8_t b[8];
    for (int i = 0; i < 8; ++i) b[i] = (uint8_t)(v >> (56 - 8 * i));
    h.update(b, 8);
}

// a device call of the library made from inside this one: its negative code leaves as this call's (status_of turns
// a DevErr back into -(100 + hipError_t) and anything else into -2)
void dev_rc(int rc) {
    if (rc <= -100) throw kzgamd::DevErr{(hipError_t)(-rc - 100)};
    if (rc < 0) throw rc;
}

bool p1_equal(const blst_p1& a, const blst_p1& b) {  // as group elements, any Z
    const ff::Fp* A = reinterpret_cast<const ff::Fp*>(&a);
    const ff::Fp* B = reinterpret_cast<const ff::Fp*>(&b);
    const bool ia = A[2].is_zero(), ib = B[2].is_zero();
    if (ia || ib) return ia && ib;
    const ff::Fp z1z1 = hfp::sqr(A[2]), z2z2 = hfp::sqr(B[2]);
    const ff::Fp u1 = hfp::mul(A[0], z2z2), u2 = hfp::mul(B[0], z1z1);
    const ff::Fp s1 = hfp::mul(A[1], hfp::mul(z2z2, B[2])), s2 = hfp::mul(B[1], hfp::mul(z1z1, A[2]));
    return !memcmp(&u1, &u2, sizeof u1) && !memcmp(&s1, &s2, sizeof s1);
}

// rows x n scalars (host) against the n points of `jac`: out[row] = sum_i scalars[row * n + i] * jac[i].  The points go
// to affine form on the GPU (the identity as (0, 0), which the engine steps over) and into a handle for this one call.
void g1_msm_rows(blst_p1* out, const blst_p1* jac, size_t n, const Fr* scalars, size_t rows, int device, const KzgAmdConfig* dev_cfg) {
    std::vector<blst_p1_affine> aff(n);
    dev_rc(kzgamd_g1_to_affine_batch(aff.data(), jac, n, dev_cfg));
    kzgamd::Options opt;
    opt.device = device;
    // the membership test where it costs less than the split saves, the unsplit engine beyond (as mult_pippenger)
    kzgamd::MsmContext* ctx = kzgamd::msm_create(aff.data(), n, false, false, false,
                                                 n <= ((size_t)1 << 15) ? kzgamd::G1_CHECK : kzgamd::G1_NO_SPLIT, &opt);
    try {
        kzgamd::msm_run_host(ctx, out, scalars, n, rows);
    } catch (...) {
        kzgamd::msm_destroy(ctx);
        throw;
    }
    kzgamd::msm_destroy(ctx);
}

}  // namespace

extern "C" int kzgamd_verify_trusted_setup(void* vntt, unsigned* failed, const blst_p1* g1_monomial, const blst_p1* g1_lagrange,
                                           const blst_p2* g2_monomial, size_t num_g1, size_t num_g2, const uint8_t seed[32],
                                           const KzgAmdConfig* cfg) {
    if (failed) *failed = 0;
    if (!g1_monomial || !g2_monomial) return -1;
    if (num_g1 < 2 || num_g2 < 2) return 2;
    NttCtx* ntt = (NttCtx*)vntt;
    const bool has_l = g1_lagrange != nullptr;
    if (has_l && (!ntt || (num_g1 & (num_g1 - 1)) || num_g1 > ntt->W)) return 3;
    int device;
    size_t slice;
    if (int rc = kzgamd::read_slice_config(cfg, "kzgamd_verify_trusted_setup", "lincomb_slice", SLICE_DEFAULT, SLICE_MIN, &device, &slice))
        return rc;
    {
        return kzgamd::status_of([&]() -> int {
            if (has_l) device = ntt->device;  // the transform runs where its handle lives
            else if (device < 0) DEV_TRY(hipGetDevice(&device));
            kzgamd::DeviceGuard on_device(device);
            DEV_TRY(on_device.err);
            KzgAmdConfig dev_cfg;  // the device alone, for the calls of other files (their keys are not this call's)
            kzgamd_config_init(&dev_cfg);
            dev_cfg.device = device;
            const blst_p1 *M = g1_monomial, *L = g1_lagrange;
            const blst_p2* Q = g2_monomial;
            const size_t n1 = num_g1, n2 = num_g2;

            // ---- the challenge
            uint8_t derived[32];
            if (!seed) {
                std::vector<uint8_t> buf(48 * n1 > 96 * n2 ? 48 * n1 : 96 * n2);
                kzgamd::Sha256 h;
                h.update((const uint8_t*)SEED_DOMAIN, sizeof SEED_DOMAIN - 1);
                put_be64(h, n1);
                put_be64(h, n2);
                const uint8_t flag = has_l ? 1 : 0;
                h.update(&flag, 1);
                dev_rc(kzgamd_g1_compress_batch(buf.data(), M, n1, &dev_cfg));
                h.update(buf.data(), 48 * n1);
                if (has_l) {
                    dev_rc(kzgamd_g1_compress_batch(buf.data(), L, n1, &dev_cfg));
                    h.update(buf.data(), 48 * n1);
                }
                dev_rc(kzgamd_g2_compress_batch(buf.data(), Q, n2, &dev_cfg));
                h.update(buf.data(), 96 * n2);
                h.finish(derived);
                seed = derived;
            }
            Fr r = hash_to_bls_field(seed);
            if (r.is_zero()) r = Fr::one();

            // ---- the powers of r, and C, D on the device
            kzgamd::CallStream s;
            const size_t npow = n1 > n2 ? n1 : n2;
            std::vector<Fr> pw(npow);
            blst_p2 CD[2];
            {
                const size_t m = n2 - 1;  // terms of C and of D
                if (slice > m) slice = m;
                ScopedBuf d_pw, d_q, d_work, d_cd;
                d_pw.alloc(npow * sizeof(Fr));
                d_q.alloc((slice + 1) * sizeof(blst_p2));
                d_work.alloc(kzgamd::g2lc_gpu::work_bytes(slice));
                d_cd.alloc(2 * sizeof(blst_p2));
                kzgamd::fr_powers_enqueue((Fr*)d_pw.p, r, Fr::one(), 0, npow, s.st);
                DEV_TRY(hipGetLastError());
                DEV_TRY(hipMemcpyAsync(pw.data(), d_pw.p, npow * sizeof(Fr), hipMemcpyDeviceToHost, s.st));
                hp::G2Jac acc[2] = {hp::g2_inf(), hp::g2_inf()};
                for (size_t at = 0; at < m; at += slice) {  // slice sums are added on the host: one slice for every m <= 2^18
                    const size_t cnt = m - at < slice ? m - at : slice;
                    DEV_TRY(hipMemcpyAsync(d_q.p, Q + at, (cnt + 1) * sizeof(blst_p2), hipMemcpyHostToDevice, s.st));
                    for (int k = 0; k < 2; ++k)  // C over Q[at ...], D over Q[at + 1 ...], the same scalars
                        kzgamd::g2lc_gpu::lincomb_enqueue((blst_p2*)d_cd.p + k, (const blst_p2*)d_q.p + k, (const Fr*)d_pw.p + at, cnt,
                                                          d_work.p, s.st);
                    DEV_TRY(hipGetLastError());
                    DEV_TRY(hipMemcpyAsync(CD, d_cd.p, sizeof CD, hipMemcpyDeviceToHost, s.st));
                    DEV_TRY(hipStreamSynchronize(s.st));
                    for (int k = 0; k < 2; ++k) {
                        hp::G2Jac part;
                        memcpy(&part, &CD[k], sizeof part);
                        acc[k] = hp::g2_add(acc[k], part);
                    }
                }
                memcpy(CD, acc, sizeof CD);
            }

            // ---- A, B and S = sum r^k M[k]: three rows over M
            std::vector<Fr> rows(3 * n1, Fr::zero());
            for (size_t i = 0; i + 1 < n1; ++i) rows[i] = rows[n1 + i + 1] = pw[i];
            for (size_t i = 0; i < n1; ++i) rows[2 * n1 + i] = pw[i];
            blst_p1 ABS[3];
            g1_msm_rows(ABS, M, n1, rows.data(), 3, device, &dev_cfg);

            unsigned bad = 0;
            // bit 1: the generators
            {
                ff::Fp gx, gy, mx, my;
                kzgamd::host_g1_generator(gx, gy);
                hp::G2Jac q0;
                memcpy(&q0, &Q[0], sizeof q0);
                if (kzgamd::host_p1_to_affine(&M[0], mx, my) || memcmp(&gx, &mx, sizeof gx) || memcmp(&gy, &my, sizeof gy) ||
                    !hp::g2_equal(q0, hp::g2_generator()))
                    bad |= 1;
            }
            // bit 2: e(B, Q[0]) == e(A, Q[1]);  bit 4: e(M[1], C) == e(M[0], D)
            if (kzgamd_pairings_verify(&ABS[1], &Q[0], &ABS[0], &Q[1]) != 1) bad |= 2;
            if (kzgamd_pairings_verify(&M[1], &CD[0], &M[0], &CD[1]) != 1) bad |= 4;
            // bit 8: sum_i f[i] L[i] == S with f the forward transform of the powers
            if (has_l) {
                std::vector<Fr> f(n1);
                const int rc = ntt_fr(ntt, (blst_fr*)f.data(), (const blst_fr*)pw.data(), n1, 0);
                dev_rc(rc);
                if (rc > 0) throw kzgamd::DevErr{hipErrorInvalidValue};
                blst_p1 lsum;
                g1_msm_rows(&lsum, L, n1, f.data(), 1, device, &dev_cfg);
                if (!p1_equal(lsum, ABS[2])) bad |= 8;
            }
            if (failed) *failed = bad;
            return bad ? 1 : 0;
        });
    }
}

extern "C" int kzgamd_verify_trusted_setup_file(void* ntt, unsigned* failed, FILE* in, const uint8_t seed[32], const KzgAmdConfig* cfg) {
    if (failed) *failed = 0;
    if (!in) return -1;
    int device;
    size_t slice;
    if (int rc = kzgamd::read_slice_config(cfg, "kzgamd_verify_trusted_setup_file", "lincomb_slice", SLICE_DEFAULT, SLICE_MIN, &device, &slice))
        return rc;
    try {
        // the text once, for the counts and then for the points
        std::string text;
        char chunk[1 << 16];
        for (size_t got; (got = fread(chunk, 1, sizeof chunk, in)) > 0;) text.append(chunk, got);
        KzgAmdConfig dev_cfg;  // the reader's one key is codec_slice: it gets the device alone
        kzgamd_config_init(&dev_cfg);
        dev_cfg.device = device;
        size_t n1 = 0, n2 = 0;
        FILE* mem = fmemopen((void*)text.data(), text.size(), "r");
        if (!mem) return -2;
        int rc = kzgamd_read_trusted_setup_file(mem, nullptr, nullptr, nullptr, &n1, &n2, &dev_cfg);
        fclose(mem);
        if (rc) return rc < 0 ? rc : 10 + rc;
        if (n1 < 2 || n2 < 2) return 2;
        std::vector<blst_p1> M(n1), L(n1);
        std::vector<blst_p2> Q(n2);
        mem = fmemopen((void*)text.data(), text.size(), "r");
        if (!mem) return -2;
        rc = kzgamd_read_trusted_setup_file(mem, M.data(), L.data(), Q.data(), &n1, &n2, &dev_cfg);
        fclose(mem);
        if (rc) return rc < 0 ? rc : 10 + rc;
        return kzgamd_verify_trusted_setup(ntt, failed, M.data(), L.data(), Q.data(), n1, n2, seed, cfg);
    } catch (...) {
        return -2;
    }
}
