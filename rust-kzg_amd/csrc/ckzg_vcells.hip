// kzgamd_verify_cell_kzg_proof_batch_many: nbatch independent verify_cell_kzg_proof_batch inputs (kzg/src/das.rs:294-389)
// in one call under ONE pairing — the data-column sidecars of a slot, each with a verdict of its own.
//
// Batch b has the reference's challenge r_b (of that batch alone) and the reference's pair
//     P_b = sum_i r_b^i proof_i,      L_b = sum_j weight_j C_j - [I_b(s)] + sum_i r_b^i h_i^64 proof_i,
// which it accepts when e(L_b, G2) == e(P_b, [s^64]G2).  With outer weights rho_b = rho^b the call checks
//     e(sum_b rho_b L_b, G2) == e(sum_b rho_b P_b, [s^64]G2).
// Everything is linear in the cell weights w_i = rho_b r_b^i, so the whole call is what ONE batch is in ckzg_7594.hip:
// one decode of [proofs | commitments, de-duplicated across the call | g1_monomial[0..64)], one aggregated
// interpolation polynomial (64 coefficients, whatever nbatch is), one two-row MSM, one download.
// Host: the r_b (SHA-256 chains, one per batch, on up to HASH_THREADS threads while the GPU takes the cells and
// decodes the points), rho, the weights and the row scalars.  GPU: the cells are uploaded as they were passed and read once by
// k_vcells_agg, which also makes the "element < r" test of every one of them.
#include "ckzg_shared.h"

#include <unordered_map>

namespace {

constexpr size_t CELLS_PER_EXT_BLOB = 2 * CELLS_PER_BLOB;  // 128
constexpr size_t BYTES_PER_CELL = CELL_SIZE * 32;
constexpr size_t SLICE = KzgAmdSettings::VCELLS_SLICE;
constexpr unsigned HASH_THREADS = 8;

// One wave per slice of at most SLICE cells of one column; lane f owns field element f, so a cell is one coalesced
// 2048-byte read (two 16-byte loads per lane).  part[p][f] = sum over the cells i of slice p of w_i * cell_i[f]: w_i in
// Montgomery form and the element canonical, so the products and their sums are canonical.  An element >= r raises
// *status and counts as zero (the call is rejected).
// slices: 2 words per slice (first position in `order`, cells); order: the cells' indices grouped by column.
__global__ void __launch_bounds__(64) k_vcells_agg(ff::Fr* __restrict__ part, int* __restrict__ status, const uint4* __restrict__ cells,
                                                   const u32* __restrict__ slices, const u32* __restrict__ order,
                                                   const ff::Fr* __restrict__ w) {
    const u32 p = blockIdx.x, f = threadIdx.x;
    const u32 start = slices[2 * p], count = slices[2 * p + 1];
    ff::Fr acc = ff::Fr::zero();
    bool bad = false;
    size_t i = order[start];
    uint4 lo = cells[(i * CELL_SIZE + f) * 2], hi = cells[(i * CELL_SIZE + f) * 2 + 1];
#pragma unroll 1
    for (u32 j = 0; j < count; ++j) {
        const u32 be[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const ff::Fr wi = w[i];
        if (j + 1 < count) {  // the next cell's bytes are on their way during this cell's product
            i = order[start + j + 1];
            lo = cells[(i * CELL_SIZE + f) * 2];
            hi = cells[(i * CELL_SIZE + f) * 2 + 1];
        }
        bool ok;
        ff::Fr c = fr_load_be(be, &ok);
        if (!ok) {
            bad = true;
            c = ff::Fr::zero();
        }
        acc = ff::add(acc, fmul(wi, c));
    }
    if (bad) *status = 1;
    part[(size_t)p * CELL_SIZE + f] = acc;
}

// agg[col][brp6(f)] = the sum of the partial rows pstart[col] .. pstart[col + 1] of column col (none: zero), the input
// of the 128 inverse transforms of 64 (k_vcell_agg's output, ckzg_7594.hip)
__global__ void __launch_bounds__(64) k_vcells_fold(ff::Fr* __restrict__ agg, const ff::Fr* __restrict__ part,
                                                    const u32* __restrict__ pstart) {
    const u32 col = blockIdx.x, f = threadIdx.x;
    ff::Fr acc = ff::Fr::zero();
    for (u32 p = pstart[col]; p < pstart[col + 1]; ++p) acc = ff::add(acc, part[(size_t)p * CELL_SIZE + f]);
    agg[col * CELL_SIZE + (__builtin_bitreverse32(f) >> 26)] = acc;
}

struct Key48 {
    const uint8_t* p;
    bool operator==(const Key48& o) const { return memcmp(p, o.p, 48) == 0; }
};
struct Key48Hash {
    size_t operator()(const Key48& k) const {
        // compressed points of different commitments differ in their x coordinate: any 8 bytes past the flag byte do
        uint64_t a, b;
        memcpy(&a, k.p + 8, 8);
        memcpy(&b, k.p + 32, 8);
        return (size_t)(a ^ (b * 0x9e3779b97f4a7c15ull));
    }
};

inline void fr_to_be32(uint8_t out[32], const ff::Fr& mont) {  // FsFr::to_bytes
    const ff::Fr c = ff::from_mont(mont);
    for (int k = 0; k < 8; ++k) {
        uint8_t* q = out + (7 - k) * 4;
        q[0] = (uint8_t)(c.v[k] >> 24);
        q[1] = (uint8_t)(c.v[k] >> 16);
        q[2] = (uint8_t)(c.v[k] >> 8);
        q[3] = (uint8_t)c.v[k];
    }
}

// the derived outer challenge: SHA-256("KZGAMD_VCELLSET1" | u64_be(nbatch) | the nbatch r_b, 32 bytes big-endian each)
ff::Fr outer_challenge(const std::vector<ff::Fr>& rb) {
    kzgamd::Sha256 h;
    uint8_t head[24];
    memcpy(head, "KZGAMD_VCELLSET1", 16);
    const uint64_t nb = rb.size();
    for (int i = 0; i < 8; ++i) head[16 + 7 - i] = (uint8_t)(nb >> (8 * i));
    h.update(head, 24);
    for (const ff::Fr& r : rb) {
        uint8_t be[32];
        fr_to_be32(be, r);
        h.update(be, 32);
    }
    uint8_t digest[32];
    h.finish(digest);
    return vc_hash_to_fr(digest);
}

// (P, L) = sum_b rho^b (P_b, L_b) of the call, into out[0], out[1]
void many_g1(blst_p1 out[2], const Bytes48* commitments_bytes, const uint64_t* cell_indices, const Cell* cells,
             const Bytes48* proofs_bytes, const uint64_t* num_cells, size_t nbatch, const blst_fr* rho_in, const CKZGSettings* cs,
             KzgAmdSettings* dev) {
    using clk = std::chrono::steady_clock;
    const clk::time_point t0 = clk::now();
    auto ms_since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    std::vector<size_t> first(nbatch + 1, 0);
    for (size_t b = 0; b < nbatch; ++b) first[b + 1] = first[b] + (size_t)num_cells[b];
    const size_t n = first[nbatch];
    memset(out, 0, 2 * sizeof(blst_p1));
    if (n == 0) return;
    CK_REQUIRE(n < ((size_t)1 << 31), "Too many cells");
    for (size_t i = 0; i < n; ++i) CK_REQUIRE(cell_indices[i] < CELLS_PER_EXT_BLOB, "Invalid cell index");
    // the commitments of the whole call, first occurrences in order: decoded and tested once
    std::vector<Bytes48> uniq;
    std::vector<u32> gidx(n);
    {
        std::unordered_map<Key48, u32, Key48Hash> seen;
        seen.reserve(256);
        for (size_t i = 0; i < n; ++i) {
            auto it = seen.find(Key48{commitments_bytes[i].bytes});
            if (it == seen.end()) {
                it = seen.emplace(Key48{commitments_bytes[i].bytes}, (u32)uniq.size()).first;  // keyed on the caller's bytes
                uniq.push_back(commitments_bytes[i]);
            }
            gidx[i] = it->second;
        }
    }
    const size_t m = uniq.size(), np = n + m + CELL_SIZE;

    std::lock_guard<std::mutex> vlk(dev->vmu);
    if (dev->mono64_bytes.empty()) {
        dev->mono64_bytes.resize(CELL_SIZE * 48);
        compress_on_host(dev->mono64_bytes.data(), cs->g1_values_monomial, CELL_SIZE);
    }
    const bool have_mono = dev->d_mono64.p != nullptr;
    const size_t ndec = have_mono ? n + m : np;
    {
        std::vector<uint8_t> stage(ndec * 48);
        memcpy(stage.data(), proofs_bytes, n * 48);
        memcpy(stage.data() + n * 48, uniq.data(), m * 48);
        if (!have_mono) memcpy(stage.data() + (n + m) * 48, dev->mono64_bytes.data(), CELL_SIZE * 48);
        vc_decode_begin(dev, stage, ndec, dev->d_mono64.p, have_mono ? CELL_SIZE : 0);
    }
    // from here on the caller's cells may be on their way to the device and the decode runs: nothing of this call may
    // stay in flight when it returns, however it returns
    struct Drain {
        KzgAmdSettings* dev;
        size_t np;
        bool armed = true;
        ~Drain() {
            if (!armed) return;
            {
                std::lock_guard<std::mutex> lk(dev->mu);
                kzgamd::DeviceGuard on_device(dev->device);
                if (on_device.err == hipSuccess) (void)hipStreamSynchronize(dev->stream);
            }
            try {
                (void)vc_decode_status(dev, np);
            } catch (...) {
            }
        }
    } drain{dev, np};

    // the r_b: batch b hashes its own de-duplicated commitments (in order of first appearance) and its cells
    std::vector<ff::Fr> rb(nbatch);
    std::atomic<size_t> next{0};
    std::atomic<bool> hash_failed{false};
    auto hash_worker = [&] {
        try {
            std::vector<u32> stamp(m, 0xffffffffu), local(m);
            std::vector<Bytes48> lu;
            std::vector<uint64_t> lidx;
            for (size_t b = next.fetch_add(1); b < nbatch; b = next.fetch_add(1)) {
                const size_t f = first[b], nc = first[b + 1] - f;
                lu.clear();
                lidx.resize(nc);
                for (size_t i = 0; i < nc; ++i) {
                    const u32 g = gidx[f + i];
                    if (stamp[g] != (u32)b) {
                        stamp[g] = (u32)b;
                        local[g] = (u32)lu.size();
                        lu.push_back(uniq[g]);
                    }
                    lidx[i] = local[g];
                }
                rb[b] = vc_challenge(lu.data(), lu.size(), lidx.data(), cell_indices + f, cells + f, proofs_bytes + f, nc);
            }
        } catch (...) {
            hash_failed = true;
        }
    };
    struct Joiner {
        std::vector<std::thread> th;
        void join() {
            for (auto& t : th)
                if (t.joinable()) t.join();
        }
        ~Joiner() { join(); }
    } hashers;
    const unsigned nthreads = (unsigned)std::min<size_t>(HASH_THREADS, nbatch);
    double* tm = dev->vm_ms;  // stage times of this call (kzgamd_vcells_timing); written under dev->vmu
    tm[0] = ms_since(t0);     // de-duplication, staging, the decode enqueued
    const clk::time_point t_hash = clk::now();
    for (unsigned t = 0; t < nthreads; ++t) hashers.th.emplace_back(hash_worker);

    // meanwhile: the cells, as they are, to the device
    {
        std::lock_guard<std::mutex> lk(dev->mu);
        kzgamd::DeviceGuard on_device(dev->device);
        DEV_TRY(on_device.err);
        dev->ensure_recover(1);
        dev->ensure_vcells_many(n);
        if (!dev->d_roots8192.p) {
            dev->d_roots8192.ensure(2 * N + 1);
            DEV_TRY(hipMemcpy(dev->d_roots8192.p, cs->roots_of_unity, (2 * N + 1) * sizeof(ff::Fr), hipMemcpyHostToDevice));
        }
        DEV_TRY(hipMemsetAsync(dev->d_vm_status.p, 0, sizeof(int), dev->stream));
        DEV_TRY(hipMemcpyAsync(dev->d_vm_cells.p, cells, n * BYTES_PER_CELL, hipMemcpyHostToDevice, dev->stream));
    }
    tm[1] = ms_since(t_hash);  // the cells handed to the copy engine
    // ... and the tables of the two kernels: the cells grouped by column (a counting sort), each column cut into slices
    const size_t T_SL = CELLS_PER_EXT_BLOB + 1;
    std::vector<u32> colstart(CELLS_PER_EXT_BLOB + 1, 0u);
    for (size_t i = 0; i < n; ++i) ++colstart[(size_t)cell_indices[i] + 1];
    for (size_t c = 0; c < CELLS_PER_EXT_BLOB; ++c) colstart[c + 1] += colstart[c];
    size_t nslices = 0;
    for (size_t c = 0; c < CELLS_PER_EXT_BLOB; ++c) nslices += (colstart[c + 1] - colstart[c] + SLICE - 1) / SLICE;
    const size_t T_ORD = T_SL + 2 * nslices;
    std::vector<u32> tab(T_ORD + n);
    {
        std::vector<u32> cursor(colstart.begin(), colstart.begin() + CELLS_PER_EXT_BLOB);
        for (size_t i = 0; i < n; ++i) tab[T_ORD + cursor[(size_t)cell_indices[i]]++] = (u32)i;
        size_t p = 0;
        for (size_t c = 0; c < CELLS_PER_EXT_BLOB; ++c) {
            tab[c] = (u32)p;
            for (u32 s0 = colstart[c]; s0 < colstart[c + 1]; s0 += (u32)SLICE, ++p) {
                tab[T_SL + 2 * p] = s0;
                tab[T_SL + 2 * p + 1] = std::min<u32>((u32)SLICE, colstart[c + 1] - s0);
            }
        }
        tab[CELLS_PER_EXT_BLOB] = (u32)p;
    }
    hashers.join();
    tm[2] = ms_since(t_hash);  // every r_b known (the upload and the tables ran beside the hashes)
    const clk::time_point t_sc = clk::now();
    if (hash_failed) throw std::bad_alloc();

    // the weights w_i = rho^b r_b^i and the two rows of scalars over [proofs | commitments | g1_monomial[0..64)]
    const ff::Fr rho = rho_in ? *reinterpret_cast<const ff::Fr*>(rho_in) : outer_challenge(rb);
    const ff::Fr* roots = reinterpret_cast<const ff::Fr*>(cs->roots_of_unity);
    ff::Fr h64[CELLS_PER_EXT_BLOB];  // h_k^64 (das.rs:837-884)
    for (size_t c = 0; c < CELLS_PER_EXT_BLOB; ++c) h64[c] = roots[reverse_bits(c, 7) * CELL_SIZE];
    std::vector<ff::Fr> sc(2 * np, ff::Fr::zero());
    ff::Fr rho_b = ff::Fr::one();
    for (size_t b = 0; b < nbatch; ++b) {
        ff::Fr w = rho_b;
        for (size_t i = first[b]; i < first[b + 1]; ++i) {
            sc[i] = w;                                                    // row 0: proofs
            sc[np + i] = ff::mul(w, h64[(size_t)cell_indices[i]]);        // row 1: w_i h^64
            sc[np + n + gidx[i]] = ff::add(sc[np + n + gidx[i]], w);      // row 1: commitment weights
            w = ff::mul(w, rb[b]);
        }
        rho_b = ff::mul(rho_b, rho);
    }
    std::vector<ff::Fr> interp(CELL_SIZE);
    int status = 0;
    tm[3] = ms_since(t_sc);  // rho, the weights, the row scalars
    const clk::time_point t_gpu = clk::now();
    {
        std::lock_guard<std::mutex> lk(dev->mu);
        kzgamd::DeviceGuard on_device(dev->device);
        DEV_TRY(on_device.err);
        hipStream_t st = dev->stream;
        const u32* d_tab = dev->d_vm_tab.p;
        DEV_TRY(hipMemcpyAsync(dev->d_vm_w.p, sc.data(), n * sizeof(ff::Fr), hipMemcpyHostToDevice, st));  // row 0 = the weights
        DEV_TRY(hipMemcpyAsync(dev->d_vm_tab.p, tab.data(), tab.size() * sizeof(u32), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_vcells_agg, dim3((unsigned)nslices), dim3(64), 0, st, dev->d_vm_part.p, dev->d_vm_status.p,
                           (const uint4*)dev->d_vm_cells.p, d_tab + T_SL, d_tab + T_ORD, (const ff::Fr*)dev->d_vm_w.p);
        hipLaunchKernelGGL(k_vcells_fold, dim3((unsigned)CELLS_PER_EXT_BLOB), dim3(64), 0, st, dev->d_rec[0].p,
                           (const ff::Fr*)dev->d_vm_part.p, d_tab);
        DEV_TRY(hipGetLastError());
        if (kzgamd_ntt_fr_device(dev->ntt.get(), dev->d_rec[1].p, dev->d_rec[0].p, CELL_SIZE, CELLS_PER_EXT_BLOB, 1, st) != 0)
            throw CkErr{C_KZG_ERROR, "ntt"};
        vc_interp_enqueue(dev->d_rec[2].p, dev->d_rec[1].p, dev->d_roots8192.p, st);
        DEV_TRY(hipMemcpyAsync(interp.data(), dev->d_rec[2].p, CELL_SIZE * sizeof(ff::Fr), hipMemcpyDeviceToHost, st));
        DEV_TRY(hipMemcpyAsync(&status, dev->d_vm_status.p, sizeof(int), hipMemcpyDeviceToHost, st));
        DEV_TRY(hipStreamSynchronize(st));
    }
    tm[4] = ms_since(t_gpu);  // weights and tables up, k_vcells_agg, k_vcells_fold, transforms, interpolation, 64 coefficients down
    CK_REQUIRE(status == 0, "Invalid scalar");
    for (size_t k = 0; k < CELL_SIZE; ++k) sc[np + n + m + k] = ff::neg(ff::to_mont(interp[k]));  // the kernels work on canonical values
    blst_p1 pl[2];
    {
        std::lock_guard<std::mutex> lk(dev->mu);
        kzgamd::DeviceGuard on_device(dev->device);
        DEV_TRY(on_device.err);
        DEV_TRY(hipEventSynchronize(dev->ev_decoded));
        if (!dev->msm_verify) dev->msm_verify.reset(kzgamd::msm_create(dev->d_vpts.p, np, true, false, true, kzgamd::G1_TRUSTED, &dev->opt));
        else kzgamd::msm_reset_points(dev->msm_verify.get(), dev->d_vpts.p, np);
        kzgamd::msm_run_host(dev->msm_verify.get(), pl, sc.data(), np, 2);
    }
    const std::vector<int> stat = vc_decode_status(dev, np);
    tm[5] = ms_since(t_gpu) - tm[4];  // waiting for the decode, the two-row MSM, the status words
    drain.armed = false;  // both streams have drained
    for (size_t i = 0; i < np; ++i) CK_REQUIRE(stat[i] != 1, "Invalid G1 encoding");
    for (size_t i = 0; i < n; ++i) CK_REQUIRE(stat[i] == 0, "Proof is not valid");
    for (size_t i = n; i < n + m; ++i) CK_REQUIRE(stat[i] == 0, "Commitment is not valid");
    if (!have_mono) {
        bool mono_ok = true;
        for (size_t i = n + m; i < np; ++i) mono_ok = mono_ok && stat[i] == 0;
        if (mono_ok) {
            std::lock_guard<std::mutex> lk(dev->mu);
            kzgamd::DeviceGuard on_device(dev->device);
            DEV_TRY(on_device.err);
            DevArray<AffPt> keep;
            keep.ensure(CELL_SIZE);
            if (hipMemcpy(keep.p, dev->d_vpts.p + n + m, CELL_SIZE * sizeof(AffPt), hipMemcpyDeviceToDevice) == hipSuccess) dev->d_mono64 = std::move(keep);
        }
    }
    memcpy(out, pl, sizeof pl);
}

bool args_ok(const Bytes48* commitments_bytes, const uint64_t* cell_indices, const Cell* cells, const Bytes48* proofs_bytes,
             const uint64_t* num_cells, size_t nbatch) {
    if (!num_cells) return false;
    bool any = false;
    for (size_t b = 0; b < nbatch; ++b) any = any || num_cells[b] != 0;
    return !any || (commitments_bytes && cell_indices && cells && proofs_bytes);
}

}  // namespace

extern "C" int kzgamd_vcells_info(size_t* slice_cells) {
    if (slice_cells) *slice_cells = SLICE;
    return 0;
}

extern "C" int kzgamd_vcells_timing(const CKZGSettings* s, double ms[8]) {
    KzgAmdSettings* dev = lookup(s);
    if (!dev || !ms) return -1;
    std::lock_guard<std::mutex> vlk(dev->vmu);
    memcpy(ms, dev->vm_ms, sizeof dev->vm_ms);
    return 0;
}

extern "C" C_KZG_RET kzgamd_verify_cell_kzg_proof_batch_many_g1(blst_p1 out[2], const Bytes48* commitments_bytes,
                                                                const uint64_t* cell_indices, const Cell* cells,
                                                                const Bytes48* proofs_bytes, const uint64_t* num_cells, size_t nbatch,
                                                                const blst_fr* rho, const CKZGSettings* s) {
    if (!out) return C_KZG_BADARGS;
    KzgAmdSettings* dev = lookup(s);
    if (!dev) return C_KZG_BADARGS;
    if (nbatch == 0) {
        memset(out, 0, 2 * sizeof(blst_p1));
        return C_KZG_OK;
    }
    if (!args_ok(commitments_bytes, cell_indices, cells, proofs_bytes, num_cells, nbatch)) return C_KZG_BADARGS;
    blst_p1 pl[2];
    const C_KZG_RET rc = guarded([&] { many_g1(pl, commitments_bytes, cell_indices, cells, proofs_bytes, num_cells, nbatch, rho, s, dev); });
    if (rc == C_KZG_OK) memcpy(out, pl, sizeof pl);
    return rc;
}

extern "C" C_KZG_RET kzgamd_verify_cell_kzg_proof_batch_many(bool* ok, bool* ok_each, const Bytes48* commitments_bytes,
                                                             const uint64_t* cell_indices, const Cell* cells,
                                                             const Bytes48* proofs_bytes, const uint64_t* num_cells, size_t nbatch,
                                                             const blst_fr* rho, const CKZGSettings* s) {
    if (!ok) return C_KZG_BADARGS;
    KzgAmdSettings* dev = lookup(s);
    if (!dev) return C_KZG_BADARGS;
    if (nbatch == 0) {
        *ok = true;
        return C_KZG_OK;
    }
    if (!args_ok(commitments_bytes, cell_indices, cells, proofs_bytes, num_cells, nbatch)) return C_KZG_BADARGS;
    bool pass = false;
    std::vector<char> each(nbatch, 1);
    const C_KZG_RET rc = guarded([&] {
        blst_p1 pl[2];
        many_g1(pl, commitments_bytes, cell_indices, cells, proofs_bytes, num_cells, nbatch, rho, s, dev);
        blst_p2 g2gen, g2s64;
        const kzgamd::pairing::G2Jac gen = kzgamd::pairing::g2_generator();
        memcpy(&g2gen, &gen, sizeof g2gen);
        memcpy(&g2s64, &dev->g2_monomial[CELL_SIZE], sizeof g2s64);
        const std::chrono::steady_clock::time_point t_pair = std::chrono::steady_clock::now();
        auto ms_since = [](std::chrono::steady_clock::time_point a) {
            return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
        };
        pass = kzgamd::pairing::pairings_verify(&pl[1], &g2gen, &pl[0], &g2s64);  // two identities (no cells at all) pass
        {
            std::lock_guard<std::mutex> vlk(dev->vmu);
            dev->vm_ms[6] = ms_since(t_pair);
            dev->vm_ms[7] = 0;
        }
        if (pass || !ok_each) return;
        const std::chrono::steady_clock::time_point t_each = std::chrono::steady_clock::now();
        // the slow path, taken only on failure: the single call's verdict per batch (many_g1 has released dev->vmu)
        size_t f = 0;
        for (size_t b = 0; b < nbatch; ++b) {
            const size_t nc = (size_t)num_cells[b];
            bool okb = true;
            if (nc) vc_verify_single(&okb, commitments_bytes + f, cell_indices + f, cells + f, proofs_bytes + f, nc, s, dev);
            each[b] = okb;
            f += nc;
        }
        std::lock_guard<std::mutex> vlk(dev->vmu);
        dev->vm_ms[7] = ms_since(t_each);
    });
    if (rc != C_KZG_OK) return rc;
    if (ok_each)
        for (size_t b = 0; b < nbatch; ++b) ok_each[b] = each[b] != 0;
    *ok = pass;
    return C_KZG_OK;
}
