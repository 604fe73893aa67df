// Shared internals of the c-kzg layer (ckzg.hip: settings object, lanes, EIP-4844 proving; ckzg_verify.hip: the verify_*
// entry points and the host pairing exports; ckzg_7594.hip: cells, FK20, recovery, cell verification; ckzg_vcells.hip:
// many cell-proof batches under one pairing).  Types and
// templates every one of them needs, and the functions one of them defines for the others (namespace ckz).
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kzg_mi355x.h"
#include "ckzg_internal.h"
#include "combine.h"
#include "config.h"
#include "device_guard.h"
#include "ff.hip.h"
#include "fr29.hip.h"
#include "g1_io.hip.h"
#include "g1w.hip.h"
#include "host_call.h"
#include "host_g1.h"
#include "host_pairing.h"
#include "msm_internal.h"
#include "ntt_internal.h"
#include "sha256.h"
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <optional>
#include <thread>

using ff::u32;
using ff::u64;
using g1::AffPt;
using kzgamd::DevArray;
using kzgamd::drop_all;

// the engine handles a settings object owns
struct MsmDeleter {
    void operator()(kzgamd::MsmContext* m) const { kzgamd::msm_destroy(m); }
};
struct NttDeleter {
    void operator()(void* n) const { kzgamd_ntt_free(n); }
};
using MsmPtr = std::unique_ptr<kzgamd::MsmContext, MsmDeleter>;
using NttPtr = std::unique_ptr<void, NttDeleter>;


// ---- the verdicts of this layer: a bad argument, a failed host allocation (thrown across the translation units, caught
// by guarded()).  A failed device call is a kzgamd::DevErr (DEV_TRY, host_call.h), here as in every layer.
struct CkErr {
    C_KZG_RET rc;
    std::string what;
};
#define CK_REQUIRE(cond, msg)                      \
    do {                                           \
        if (!(cond)) throw CkErr{C_KZG_BADARGS, msg}; \
    } while (0)

constexpr size_t N = FIELD_ELEMENTS_PER_BLOB;
constexpr size_t NUM_G2 = 65;
constexpr size_t CELL_SIZE = 64;                 // FIELD_ELEMENTS_PER_CELL
constexpr size_t CELLS_PER_BLOB = N / CELL_SIZE;  // 64; the extended blob has 128 cells


// ---- Fr helpers for the proving kernel (Montgomery, 8 x u32) ----
static __device__ __forceinline__ ff::Fr fr_load_be(const u32* __restrict__ w8, bool* ok) {
    // 32 big-endian bytes -> canonical limbs; *ok = value < r
    ff::Fr a;
#pragma unroll
    for (int k = 0; k < 8; ++k) a.v[k] = __builtin_bswap32(w8[7 - k]);
    u64 borrow = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        u64 d = (u64)a.v[k] - ff::FrParams::p(k) - borrow;
        borrow = (d >> 32) & 1;
    }
    *ok = borrow != 0;
    return a;
}
// Montgomery inverse by binary Euclid (ff.hip.h); 0 -> 0 like blst_fr_eucl_inverse
static __device__ ff::Fr fr_inverse(const ff::Fr& a) { return ff::inverse_bgcd(a); }
// ff::mul on blst_fr values through the 29-bit multiplier of the NTT (fr29::mul_blst: the same result in about half
// the instructions); the quotient kernels below are a stream of such products
static __device__ __forceinline__ ff::Fr fmul(const ff::Fr& a, const ff::Fr& b) { return fr29::mul_blst(a, b); }


// Host worker threads for the per-blob SHA-256 challenges of a batch, kept alive between calls: spawning 16
// threads costs ~0.4 ms, a tenth of a 256-blob proof call.
class WorkerPool {
  public:
    explicit WorkerPool(unsigned n) {
        for (unsigned w = 0; w < n; ++w) th_.emplace_back([this, w] { loop(w); });
    }
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    unsigned size() const { return (unsigned)th_.size(); }
    // runs fn(w) for w = 0 .. active-1 on the pool and returns when all are done
    void run(unsigned active, const std::function<void(unsigned)>& fn) {
        std::unique_lock<std::mutex> lk(m_);
        job_ = &fn;
        active_ = active;
        pending_ = (unsigned)th_.size();
        ++gen_;
        cv_.notify_all();
        done_.wait(lk, [this] { return pending_ == 0; });
        job_ = nullptr;
    }

  private:
    void loop(unsigned w) {
        unsigned seen = 0;
        for (;;) {
            const std::function<void(unsigned)>* job;
            unsigned active;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                job = job_;
                active = active_;
            }
            if (w < active) (*job)(w);
            {
                std::lock_guard<std::mutex> lk(m_);
                if (--pending_ == 0) done_.notify_all();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(unsigned)>* job_ = nullptr;
    unsigned active_ = 0, pending_ = 0, gen_ = 0;
    bool stop_ = false;
};

constexpr int QT = 512;            // threads per blob
// cell proofs by FK20 from this batch size.  Re-measured after the G1 stages were rewritten (round 4, tools/time_cells.py,
// one settings object per form): 1 / 2 / 3 / 4 / 8 / 16 blobs FK20 4.15 / 4.16 / 4.23 / 4.25 / 4.29 / 5.32 ms, direct form
// 1.91 / 3.16 / 4.52 / 5.75 / 10.88 / 20.65 ms (round 3's crossover was 16 blobs at 25 ms either way)
constexpr size_t FK20_MIN_BLOBS = 3;
constexpr size_t PROVE_CHUNK = 64;  // blobs per pipeline stage of a large compute_blob_kzg_proof batch
constexpr size_t COMMIT_CHUNK = 64;   // smallest pipeline stage of a blob_to_kzg_commitment batch (batches from twice this are pipelined)
constexpr size_t QSPLIT_MAX = 16;  // up to this many blobs (a lane batch) run the multi-workgroup variant (k_quotient_a/b)
constexpr int QE = (int)(N / QT);  // elements per thread (8), element index i = k*QT + t

// decode + membership test of np compressed points: up to WIDE_CHECK_MAX points the test runs one wave per point
constexpr size_t WIDE_CHECK_MAX = 4096;
constexpr size_t WIDE_COMMIT_CHECK_MAX = 512;  // ... the commitments of a proof batch: up to this many

// see ckzg.hip
// batches up to this size leave the device as Jacobian points and are compressed on the host with one inversion
// (host_p1_compress_batch): k_final's one-lane inversion is 0.25 ms of latency, worth paying only when a block of 64
// points shares it
constexpr size_t HOST_COMPRESS_MAX = 16;
constexpr size_t HOST_CHECK_MAX = 64;  // commitments of a proof batch validated on the host's cores up to this many


// ---------------------------------------------------------------- settings object
struct CommitReq;  // ckzg.hip: the requests of the coalesced single-blob entry points
struct ProofReq;
struct KzgAmdSettings {
    int device = 0;
    MsmPtr msm_owned;                   // prepared over g1_lagrange_brp: the root's
    kzgamd::MsmContext* msm = nullptr;  // ... as every object reads it (a lane: its parent's)
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // commitment validation runs beside the proving pipeline
    // EIP-7594 state, built on first use
    DevArray<AffPt> d_monomial;               // g1_values_monomial as table slots
    MsmPtr msm_monomial;
    MsmPtr msm_xext;  // FK20: the 128 columns of 64 points of x_ext_fft_columns, one wide table
    DevArray<ff::Fr> d_fk_a, d_fk_b;  // FK20: n x 64 x 128 Toeplitz vectors / their transforms
    DevArray<g1::Xyzz> d_fk_h, d_fk_h2;  // FK20: n x 128 points, and the transform scratch
    // Every ensure_* below releases its whole group before it allocates any of it: a settings object sits beside a
    // 137 GB table, and growing the members one at a time would raise the peak by the old size of the rest.
    size_t cap_fk = 0;
    void ensure_fk20(size_t nblobs) {
        if (nblobs <= cap_fk) return;
        cap_fk = 0;
        drop_all(d_fk_a, d_fk_b, d_fk_h, d_fk_h2);
        d_fk_a.ensure(nblobs * 8192);
        d_fk_b.ensure(nblobs * 8192);
        d_fk_h.ensure(nblobs * 128);
        d_fk_h2.ensure(nblobs * 128);
        cap_fk = nblobs;
    }
    // the 128 quotient vectors per blob of the direct cell-proof path (16 MB per blob)
    void ensure_q(size_t nblobs) { d_q.ensure(nblobs * 128 * N * 8); }
    // Lanes: the reference's callers share one settings object between rayon workers (kzg/src/eip_4844.rs:781-805).
    // A host-buffer call of a few blobs takes the first idle lane — a settings object of its own for everything a call
    // mutates (streams, staging buffers, mutex) that BORROWS the tables and engine handles of its parent — so that up to
    // MAX_LANES + 1 small calls are in flight on the GPU at once (their kernels are a few hundred waves each) instead
    // of queueing on one mutex.  Lane objects are created on demand and live as long as the parent.
    static constexpr size_t LANE_MAX_BLOBS = 16;
    static constexpr int MAX_LANES = 15;
    // Coalescing of concurrent single-blob calls (one queue per entry point, combine.h): callers push a request; up to
    // `leaders` of them at a time take everything queued (up to LANE_MAX_BLOBS requests) and run it as ONE batch on a
    // lane, so that the ~10 runtime operations of a pipeline invocation (each of them takes a device-wide lock inside
    // the HIP runtime: ~100 us of serialised host time per invocation) are paid per batch, not per call.
    // Tuning keys leaders / gather_min / gather_us (apply_options).
    kzgamd::CombineQueue<CommitReq> q_commit;
    kzgamd::CombineQueue<ProofReq> q_blob_proof, q_proof;
    // the tuning keys of config.h this layer reads, copied once when the settings object is created (apply_options;
    // lanes take their parent's)
    kzgamd::Options opt;
    bool cfg_device_sha = false;
    int cfg_sha_lanes = 0;  // lanes per blob of the device Fiat-Shamir hash (tuning key sha_lanes; 0 = by batch size)
    size_t cfg_host_check_max = 64;  // see HOST_CHECK_MAX
    size_t cfg_prove_chunk = 0;
    bool cfg_wide_check = true;      // false: single-lane tests
    size_t cfg_prove_first = 0, cfg_commit_first = 0, cfg_commit_chunk = 0;
    int cfg_fk20 = -1;               // -1: by batch size
    void apply_options(const kzgamd::Options& o) {
        using namespace kzgamd;
        opt = o;
        auto configure = [&o](auto& q) {
            q.max_leaders = (int)o.t[T_LEADERS];
            q.batch_max = LANE_MAX_BLOBS;
            q.gather_min = (size_t)o.t[T_GATHER_MIN];
            q.gather_us = (int)o.t[T_GATHER_US];
        };
        configure(q_commit);
        configure(q_blob_proof);
        configure(q_proof);
        cfg_device_sha = o.t[T_DEVICE_SHA] != 0;
        cfg_sha_lanes = (int)o.t[T_SHA_LANES];
        cfg_host_check_max = (size_t)o.t[T_HOST_CHECK_MAX];
        cfg_prove_chunk = (size_t)o.t[T_PROVE_CHUNK];
        cfg_wide_check = o.t[T_WIDE_CHECK] != 0;
        cfg_prove_first = (size_t)o.t[T_PROVE_FIRST];
        cfg_commit_first = (size_t)o.t[T_COMMIT_FIRST];
        cfg_commit_chunk = (size_t)o.t[T_COMMIT_CHUNK];
        cfg_fk20 = (int)o.t[T_FK20];
    }
    std::atomic<bool> busy{false};
    // page-locked staging for calls of up to LANE_MAX_BLOBS blobs: copies to and from it are truly asynchronous (a
    // copy from / to the caller's pageable memory goes through the runtime's own staging path, which serialises
    // concurrent callers)
    unsigned char* h_in = nullptr;   // LANE_MAX_BLOBS blobs
    unsigned char* h_res = nullptr;  // per blob: 144 B result + 32 B y + 4 B status + 4 B commitment status
    void ensure_pinned() {
        if (h_in) return;
        DEV_TRY(hipHostMalloc((void**)&h_in, LANE_MAX_BLOBS * BYTES_PER_BLOB, hipHostMallocDefault));
        DEV_TRY(hipHostMalloc((void**)&h_res, LANE_MAX_BLOBS * 256, hipHostMallocDefault));
    }
    // Page-locked blob slots for the callers of the coalesced entry points: a caller copies its blob into a slot on its
    // own thread (in parallel with the other callers) before it queues its request; the batch's kernels read the
    // slots in place.  The pool belongs to the root settings object; a caller that finds it empty leaves the copy
    // to the leader (the lane's own staging).  All NSLOTS are pinned with the first caller.
    static constexpr int NSLOTS = 48;
    std::optional<kzgamd::SlotPool<kzgamd::PinnedMapped>> slots;  // the root's only, made once its device is known
    std::mutex lanes_mu;
    std::vector<std::unique_ptr<KzgAmdSettings>> lanes;
    std::atomic<unsigned> lane_rr{0};
    NttPtr ntt;                               // kzgamd_ntt_new(13)
    DevArray<ff::Fr> d_roots8192;             // roots_of_unity[0..=8192], Montgomery
    DevArray<ff::Fr> d_fr_a, d_fr_b, d_fr_ext;  // 4096, 4096, 8192 per blob
    DevArray<u32> d_cells;
    DevArray<u32> d_q;                        // 128 x 4096 x 8 per blob
    DevArray<unsigned char> d_proofs;
    size_t cap_cells = 0;
    DevArray<int> d_cstatus;
    DevArray<AffPt> d_cpts;  // decoded commitments of a proof batch of <= WIDE_COMMIT_CHECK_MAX blobs (wide check)
    std::mutex mu;
    // staging for the host-buffer entry points
    DevArray<unsigned char> d_blobs;
    DevArray<u32> d_scalars;
    DevArray<int> d_status;
    DevArray<unsigned char> d_out;
    DevArray<u32> d_z;               // n x 32 B big-endian evaluation points
    DevArray<u32> d_y;               // n x 8 u32 canonical y
    DevArray<unsigned char> d_commit;   // n x 48 B
    DevArray<unsigned char> d_qscratch;   // k_quotient_a/b scratch for up to QSPLIT_MAX blobs
    size_t cap_blobs = 0;
    std::unique_ptr<WorkerPool> pool;  // created by the first batched proof call
    // extra streams for the chunk pipeline of large proof batches (created on first use); chunk k runs on
    // pipe_stream(k), `stream` waits for all of them in pipe_join()
    static constexpr int NPIPE = 4;
    hipStream_t pipe[NPIPE] = {};
    hipEvent_t pipe_ev[NPIPE] = {};
    hipEvent_t ev_commit = nullptr;  // the commitments of a proof batch are on the device (recorded on stream2)
    hipEvent_t ev_cells = nullptr;   // the cells of a cells-and-proofs call are ready (recorded on stream; stream2 copies them out)
    // batched verification: staging for [proofs | commitments | G] and the variable-base handle over them, kept
    // between calls (a fresh handle per call cost 1.7 ms of stream / allocation / free round trips)
    std::mutex vmu;                 // one batched verification at a time per settings object (its staging buffers)
    std::vector<uint8_t> vstage;    // host staging of the 2n + 1 compressed points (must outlive the async copy)
    DevArray<unsigned char> d_vbytes;
    DevArray<AffPt> d_vpts;
    DevArray<int> d_vstat;
    hipEvent_t ev_decoded = nullptr;  // the points of a verification call are decoded (their membership test may still run)
    size_t vcap = 0;
    MsmPtr msm_verify;
    void ensure_verify(size_t np) {
        if (np <= vcap) return;
        vcap = 0;
        drop_all(d_vbytes, d_vpts, d_vstat);
        const size_t cap = np < 257 ? 257 : np;
        d_vbytes.ensure(cap * 48);
        d_vpts.ensure(cap);
        d_vstat.ensure(cap);
        vcap = cap;
    }
    hipStream_t pipe_stream(size_t k) {
        const int j = (int)(k % NPIPE);
        if (!pipe[j]) {
            if (hipStreamCreateWithFlags(&pipe[j], hipStreamNonBlocking) != hipSuccess) {
                pipe[j] = nullptr;
                return stream;
            }
            (void)hipEventCreateWithFlags(&pipe_ev[j], hipEventDisableTiming);
        }
        return pipe[j];
    }
    void pipe_join() {
        for (int j = 0; j < NPIPE; ++j)
            if (pipe[j] && pipe_ev[j]) {
                (void)hipEventRecord(pipe_ev[j], pipe[j]);
                (void)hipStreamWaitEvent(stream, pipe_ev[j], 0);
            }
    }
    // EIP-7594 cell verification / recovery state, built on first use
    std::vector<uint8_t> mono64_bytes;  // g1_values_monomial[0..64) compressed (the interpolation-polynomial commitment)
    DevArray<AffPt> d_mono64;           // ... decoded and subgroup-checked once, as MSM slots
    DevArray<ff::Fr> d_rec[4];       // recovery: four vectors of 8192 field elements per blob
    DevArray<u32> d_rec_in;          // up to 128 cells per blob (the single call: canonical limbs; a batch: the bytes as given)
    DevArray<u32> d_rec_idx;         // the single call's cell indices (128)
    DevArray<u32> d_rec_info;        // a batch: 8 words per blob (ckzg_7594.hip, RecBlob)
    size_t cap_rec = 0;              // blobs d_rec / d_rec_in / d_rec_info hold
    DevArray<ff::Fr> d_pow7;         // 7^i and 7^-i, i < 8192 (coset shifts, das.rs:463-491)
    DevArray<ff::Fr> d_pow7inv;
    bool fk20_unavailable = false;   // the FK20 table could not be built (no HBM left): batches use the direct form
    // verify_cell_kzg_proof_batch: the cells (canonical limbs), their columns and the powers of r, for k_vcell_agg
    DevArray<u32> d_vc_cells;
    DevArray<u32> d_vc_cols;
    DevArray<ff::Fr> d_vc_pw;
    size_t cap_vc = 0;
    void ensure_vcells(size_t n) {
        if (n <= cap_vc) return;
        cap_vc = 0;
        drop_all(d_vc_cells, d_vc_cols, d_vc_pw);
        const size_t cap = n < 128 ? 128 : n;
        d_vc_cells.ensure(cap * CELL_SIZE * 8);
        d_vc_cols.ensure(cap + 2 * CELLS_PER_BLOB + 1);
        d_vc_pw.ensure(cap);
        cap_vc = cap;
    }
    // kzgamd_verify_cell_kzg_proof_batch_many (ckzg_vcells.hip): the cells as the caller passed them, the weights
    // rho^b r_b^i, the tables of k_vcells_agg / k_vcells_fold ([129 partial-row starts | 2 words per slice | the cells
    // grouped by column]), one partial row of 64 sums per slice, and the "an element is >= r" word
    static constexpr size_t VCELLS_SLICE = 8;  // cells per wave of k_vcells_agg (kzgamd_vcells_info)
    DevArray<unsigned char> d_vm_cells;
    DevArray<ff::Fr> d_vm_w;
    DevArray<u32> d_vm_tab;
    DevArray<ff::Fr> d_vm_part;
    DevArray<int> d_vm_status;
    size_t cap_vm = 0;
    double vm_ms[8] = {};  // host wall time of the stages of the last such call (kzgamd_vcells_timing)
    static size_t vcells_many_slices(size_t n) { return n / VCELLS_SLICE + 2 * CELLS_PER_BLOB; }  // at most, for n cells
    void ensure_vcells_many(size_t n) {
        if (n <= cap_vm) return;
        cap_vm = 0;
        drop_all(d_vm_cells, d_vm_w, d_vm_tab, d_vm_part, d_vm_status);
        const size_t cap = n < 128 ? 128 : n, ns = vcells_many_slices(cap);
        d_vm_cells.ensure(cap * CELL_SIZE * 32);
        d_vm_w.ensure(cap);
        d_vm_tab.ensure(2 * CELLS_PER_BLOB + 1 + 2 * ns + cap);
        d_vm_part.ensure(ns * CELL_SIZE);
        d_vm_status.ensure(1);
        cap_vm = cap;
    }
    // the coset tables and the single call's index buffer once; the per-blob buffers for nblobs blobs (kept, grown on demand)
    void ensure_recover(size_t nblobs) {
        if (!d_pow7inv.p) {
            d_rec_idx.ensure(128);
            d_pow7.ensure(2 * N);
            d_pow7inv.ensure(2 * N);
            std::vector<ff::Fr> p(2 * N), q(2 * N);
            ff::Fr seven = ff::Fr::zero();
            seven.v[0] = 7;
            seven = ff::to_mont(seven);
            const ff::Fr inv7 = ff::inverse_bgcd(seven);
            p[0] = q[0] = ff::Fr::one();
            for (size_t i = 1; i < 2 * N; ++i) {
                p[i] = ff::mul(p[i - 1], seven);
                q[i] = ff::mul(q[i - 1], inv7);
            }
            DEV_TRY(hipMemcpy(d_pow7.p, p.data(), p.size() * sizeof(ff::Fr), hipMemcpyHostToDevice));
            DEV_TRY(hipMemcpy(d_pow7inv.p, q.data(), q.size() * sizeof(ff::Fr), hipMemcpyHostToDevice));
        }
        if (nblobs <= cap_rec) return;
        cap_rec = 0;
        drop_all(d_rec[0], d_rec[1], d_rec[2], d_rec[3], d_rec_in, d_rec_info);
        for (int k = 0; k < 4; ++k) d_rec[k].ensure(nblobs * 2 * N);
        d_rec_in.ensure(nblobs * 2 * N * 8);
        d_rec_info.ensure(nblobs * 8);
        cap_rec = nblobs;
    }
    std::vector<kzgamd::pairing::G2Jac> g2_monomial;  // [tau^i]G2, i < 65 (host; the pairing checks use [1])
    std::vector<ff::Fr> brp_roots;  // brp_roots_of_unity[0..8192) (host copy, Montgomery)
    DevArray<ff::Fr> brp_roots_owned;       // first 4096 = the blob evaluation domain: the root's
    const ff::Fr* d_brp_roots = nullptr;    // ... as every object reads it (a lane: its parent's)
    // Streams, events and page-locked memory go by hand; the engine handles and the device arrays free themselves
    // afterwards (hipFree synchronises the device: a stream that is gone does not matter to it).
    ~KzgAmdSettings() {
        lanes.clear();  // before the handles they borrow go away
        if (h_in) (void)hipHostFree(h_in);
        if (h_res) (void)hipHostFree(h_res);
        if (ev_commit) (void)hipEventDestroy(ev_commit);
        if (ev_cells) (void)hipEventDestroy(ev_cells);
        if (ev_decoded) (void)hipEventDestroy(ev_decoded);
        for (int j = 0; j < NPIPE; ++j) {
            if (pipe_ev[j]) (void)hipEventDestroy(pipe_ev[j]);
            if (pipe[j]) (void)hipStreamDestroy(pipe[j]);
        }
        if (stream2 && stream2 != stream) (void)hipStreamDestroy(stream2);
        if (stream) (void)hipStreamDestroy(stream);
    }
    void ensure_cells(size_t nblobs) {
        if (nblobs <= cap_cells) return;
        cap_cells = 0;
        drop_all(d_fr_a, d_fr_b, d_fr_ext, d_cells, d_q, d_proofs);
        d_fr_a.ensure(nblobs * N);
        d_fr_b.ensure(nblobs * N);
        d_fr_ext.ensure(nblobs * 2 * N);
        d_cells.ensure(nblobs * 2 * N * 8);
        d_proofs.ensure(nblobs * 128 * 48);
        cap_cells = nblobs;
    }
    void ensure(size_t nblobs) {
        if (nblobs <= cap_blobs) return;
        cap_blobs = 0;
        drop_all(d_blobs, d_scalars, d_status, d_out, d_z, d_y, d_commit, d_cstatus, d_cpts);
        d_blobs.ensure(nblobs * BYTES_PER_BLOB);
        d_scalars.ensure(nblobs * BYTES_PER_BLOB / 4);
        d_status.ensure(nblobs);
        d_out.ensure(nblobs * 144);  // 48-byte compressed results, or Jacobian for the small-batch path
        d_z.ensure(nblobs * 8);
        d_y.ensure(nblobs * 8);
        d_commit.ensure(nblobs * 48);
        d_cstatus.ensure(nblobs);
        d_cpts.ensure(WIDE_COMMIT_CHECK_MAX);
        cap_blobs = nblobs;
    }
};

namespace ckz {
// ---- the scanners of the trusted-setup text (kzg/src/eip_4844.rs:151-228), for ckzg.hip and codec.hip
inline bool is_ws(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }
inline int hexval(unsigned char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}
inline bool scan_number(const std::string& s, size_t& off, size_t& out) {
    while (off < s.size() && is_ws((unsigned char)s[off])) ++off;
    if (off >= s.size()) return false;
    size_t start = off;
    while (off < s.size() && s[off] >= '0' && s[off] <= '9') ++off;
    if (off >= s.size() || off == start || off - start > 18) return false;
    out = 0;
    for (size_t i = start; i < off; ++i) out = out * 10 + (size_t)(s[i] - '0');
    return true;
}
inline bool scan_hex_byte(const std::string& s, size_t& off, uint8_t& out) {
    while (off < s.size() && is_ws((unsigned char)s[off])) ++off;
    if (off >= s.size()) return false;
    int hi = hexval((unsigned char)s[off]);
    if (hi < 0) return false;
    if (off + 1 < s.size() && hexval((unsigned char)s[off + 1]) >= 0) {
        out = (uint8_t)(hi * 16 + hexval((unsigned char)s[off + 1]));
        off += 2;
    } else {
        out = (uint8_t)hi;
        off += 1;
    }
    return true;
}
// ---- defined in ckzg.hip
KzgAmdSettings* lookup(const CKZGSettings* s);
KzgAmdSettings* make_lane(KzgAmdSettings* parent);
// decode + membership test of np compressed points (k_decode_g1_wide / k_affpts_in_g1_wide or the single-lane kernel)
void decode_check_enqueue(g1::AffPt* d_pts, int* d_stat, const unsigned char* d_bytes, size_t np, hipStream_t st, bool wide,
                          hipEvent_t decoded = nullptr);
// for codec.hip: the decode with (`check`) or without the membership test, in the form the count picks (wide up to
// WIDE_CHECK_MAX points, the single-lane kernel above), and k_affpt_to_blst_p1 over the decoded slots
void decode_enqueue(g1::AffPt* d_pts, int* d_stat, const unsigned char* d_bytes, size_t np, hipStream_t st, bool check);
void affpt_to_blst_p1_enqueue(void* d_p1, const g1::AffPt* d_pts, size_t np, hipStream_t st);
void compress_on_host(uint8_t* out48, const blst_p1* jac, size_t n);
bool host_blob_valid(const uint8_t* blob);
void prove_batch(KZGProof* proofs, Bytes32* ys, const Blob* blobs, const Bytes32* zs, const Bytes48* commitments, size_t n,
                 KzgAmdSettings* dev, Bytes32* zs_out = nullptr, bool commitments_checked_elsewhere = false);
// ---- defined in ckzg_verify.hip
void verify_g1_begin(const Bytes48* commitments, const Bytes48* proofs, size_t n, KzgAmdSettings* dev);
void verify_g1_finish(blst_p1* proof_lincomb, blst_p1* rhs, const Bytes48* commitments, const Bytes32* zs, const Bytes32* ys, const Bytes48* proofs, size_t n, KzgAmdSettings* dev);
// ---- defined in ckzg_7594.hip: what verify_cell_kzg_proof_batch is made of, for ckzg_vcells.hip
// compute_verify_cell_kzg_proof_batch_challenge (das.rs:391-452) on the caller's bytes, Montgomery form
ff::Fr vc_challenge(const Bytes48* commitments, size_t ncommit, const uint64_t* commitment_indices, const uint64_t* cell_indices,
                    const Cell* cells, const Bytes48* proofs, size_t ncells);
ff::Fr vc_hash_to_fr(const uint8_t digest[32]);  // hash_to_bls_field
// decode + both tests of np compressed points on stream2 into dev->d_vpts / d_vstat, `ntail` ready slots appended;
// the status words (0 ok, 1 not an encoding of a curve point, 2 outside G1) once stream2 has drained.  Caller holds dev->vmu.
void vc_decode_begin(KzgAmdSettings* dev, const std::vector<uint8_t>& bytes, size_t np, const g1::AffPt* tail, size_t ntail);
std::vector<int> vc_decode_status(KzgAmdSettings* dev, size_t np);
// out[k] = sum_col v[col][k] h_col^-k, k < 64 (k_vcell_interp): enqueue only
void vc_interp_enqueue(ff::Fr* out, const ff::Fr* v, const ff::Fr* roots8192, hipStream_t st);
// verify_cell_kzg_proof_batch of n > 0 cells (takes dev->vmu)
void vc_verify_single(bool* ok, const Bytes48* commitments_bytes, const uint64_t* cell_indices, const Cell* cells,
                      const Bytes48* proofs_bytes, size_t n, const CKZGSettings* cs, KzgAmdSettings* dev);
}  // namespace ckz
using namespace ckz;

// The settings object a small host-buffer call runs on: the parent if idle, else an idle lane, else a new lane, else
// (all MAX_LANES busy) one of them in turn — its mutex queues the call.  Released by the destructor.
struct LaneRef {
    KzgAmdSettings* use = nullptr;
    bool flagged = false;
    LaneRef(KzgAmdSettings* dev, size_t nblobs) {
        use = dev;
        if (nblobs > KzgAmdSettings::LANE_MAX_BLOBS) {
            // large batches: the parent's own pipeline, one at a time (its mutex); marked busy so that small calls go
            // to the lanes meanwhile
            flagged = !dev->busy.exchange(true);
            return;
        }
        // small calls run on lanes (their streams have MSM workspaces of their own: no cross-stream events per enqueue);
        // the parent stays free for large batches
        bool expect = false;
        std::lock_guard<std::mutex> lk(dev->lanes_mu);
        for (auto& ln : dev->lanes) {
            expect = false;
            if (ln->busy.compare_exchange_strong(expect, true)) {
                use = ln.get();
                flagged = true;
                return;
            }
        }
        if ((int)dev->lanes.size() < KzgAmdSettings::MAX_LANES) {
            use = make_lane(dev);  // created busy
            flagged = true;
            return;
        }
        use = dev->lanes[dev->lane_rr.fetch_add(1) % dev->lanes.size()].get();
    }
    ~LaneRef() {
        if (flagged) use->busy.store(false);
    }
    LaneRef(const LaneRef&) = delete;
    LaneRef& operator=(const LaneRef&) = delete;
};

inline size_t reverse_bits(size_t v, unsigned bits) {
    size_t r = 0;
    for (unsigned b = 0; b < bits; ++b)
        if (v & ((size_t)1 << b)) r |= (size_t)1 << (bits - 1 - b);
    return r;
}

inline bool fr_from_be32_checked(ff::Fr& out, const uint8_t* in) {  // FsFr::from_bytes: canonical limbs, false if >= r
    for (int i = 0; i < 8; ++i) {
        const uint8_t* q = in + (7 - i) * 4;
        out.v[i] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
    }
    u64 borrow = 0;
    for (int k = 0; k < 8; ++k) {
        u64 d = (u64)out.v[k] - ff::FrParams::p(k) - borrow;
        borrow = (d >> 32) & 1;
    }
    return borrow != 0;
}

// the text of a failed call on stderr under KZGAMD_DEBUG: read when a call fails, not once per process, so that a caller
// (or a test) can turn the texts on for one call
inline void debug_text(const char* what, const char* detail = nullptr) {
    if (getenv("KZGAMD_DEBUG") != nullptr) fprintf(stderr, "kzg_mi355x: %s%s%s\n", what, detail ? ": " : "", detail ? detail : "");
}

template <class F>
C_KZG_RET guarded(F&& f) {
    try {
        f();
        return C_KZG_OK;
    } catch (const CkErr& e) {
        debug_text(e.what.c_str());
        return e.rc == C_KZG_MALLOC ? C_KZG_MALLOC : C_KZG_BADARGS;  // the reference maps every failure to BadArgs
    } catch (const kzgamd::DevErr& e) {  // of this layer or of an engine below it (MSM, NTT, fft_g1)
        debug_text(e.what, hipGetErrorString(e.e));
        return C_KZG_BADARGS;
    } catch (const std::bad_alloc&) {
        return C_KZG_MALLOC;
    } catch (...) {
        return C_KZG_BADARGS;
    }
}
