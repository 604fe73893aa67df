// Shared between ntt.hip (Fr transforms) and fftg1.hip (G1-valued transforms): the context object
// behind the opaque handle of kzgamd_ntt_new().
#pragma once
#include <hip/hip_runtime.h>
#include <map>
#include <mutex>
#include <optional>
#include <vector>

#include "combine.h"
#include "ff.hip.h"
#include "host_call.h"

// device copy of one tile plan (ntt_plan.h): the per-thread element table of every round + per-round constants
struct NttPlanDev {
    kzgamd::DevBuf d_tab;
    int nrounds = 0;
    unsigned rd[12][6];  // element bit, its LDS position bit, pos, M, barrier_after, flags (fused DAS plans)
};

namespace kzgamd {
struct Options;
// one scalar (a root, n^-1, an FK20 coefficient) split for the two lanes of a G1 scalar multiplication: the 127-bit
// magnitudes of its GLV halves (glv.hip.h) and their signs
struct RootSplit {
    ff::u32 k[2][4];
    ff::u32 neg[2];
    ff::u32 pad[2];
};
static_assert(sizeof(RootSplit) == 48, "RootSplit");
}  // namespace kzgamd

struct NttCtx {
    using Fr = ff::Fr;
    std::map<int, NttPlanDev> plans;  // key = kind * 16 + T (kind 3: fused DAS plans); filled by kzgamd_ntt_new, read-only afterwards
    int device = 0;
    unsigned scale = 0;
    size_t W = 0;
    kzgamd::DevBuf d_roots;  // W + 1 twiddles in the 2^261 domain as 9 x 29-bit limbs (Fr transforms), natural order
    kzgamd::DevBuf d_tw_fwd, d_tw_inv;  // the same, stage-major (forward roots / inverse roots)
    std::vector<Fr> roots;  // host copy, blst Montgomery form
    hipStream_t stream = nullptr;
    std::mutex mu;
    kzgamd::DevArray<Fr> d_a, d_b;
    // G1-valued transforms (fftg1.hip): the roots as GLV-split scalars, staging and work buffers
    kzgamd::DevArray<kzgamd::RootSplit> d_kroots;  // W + 1
    kzgamd::DevBuf d_p1, d_pts, d_tab;  // blst_p1 / g1::Xyzz, in bytes
    size_t cap_g1 = 0;                  // points d_p1 / d_pts hold
    // G1 stages (fftg1.hip) by their number of half-butterflies: up to g1_wide_max a wave each (limb-parallel), up to
    // g1_quad_max four lanes each, up to g1_pair_max two lanes each, one lane each above
    // (tuning keys g1_wide_max / g1_quad_max / g1_pair_max, read at creation; 0 disables a form)
    size_t g1_wide_max = 4096, g1_quad_max = 16384, g1_pair_max = 32768;

    // Combining of concurrent host-buffer calls (ntt_fr, das_fft_extension) on ONE handle — the reference shares its
    // FFTSettings by reference between rayon workers.  A caller copies its input into a page-locked slot on its own thread
    // and queues a request (combine.h); a leader takes everything queued of the same kind and length (up to COMB_MAX
    // requests) and runs it as ONE batched launch: a kernel gathers the inputs from the slots over PCIe, the batched
    // transform runs, a kernel writes the results back into the slots; every caller copies its result out of its slot.
    // A 4096-point transform is 4 us of GPU under ~60 us of copies, launches and a synchronisation: per batch instead of
    // per call.  Lists longer than COMB_NMAX, and callers that find no slot, take the plain path.
    struct HostCall : kzgamd::CombineRequest {
        size_t n;
        int kind;  // 0 forward, 1 inverse, 2 DAS extension
        unsigned char* slot;
        int rc = 0;
        HostCall(size_t n_, int kind_, unsigned char* slot_) : n(n_), kind(kind_), slot(slot_) {}
    };
    static constexpr size_t COMB_MAX = 32, COMB_NMAX = 8192;
    static constexpr int COMB_SLOTS = 40, COMB_LANES = 2;
    struct CombLane {
        hipStream_t st = nullptr;
        kzgamd::DevArray<Fr> d_in, d_out, d_tmp;  // COMB_MAX x COMB_NMAX elements each
    };
    kzgamd::CombineQueue<HostCall> comb;  // COMB_LANES leaders, batches of COMB_MAX, no gather wait
    CombLane lanes[COMB_LANES];
    std::optional<kzgamd::SlotPool<kzgamd::PinnedMapped>> slots;  // COMB_SLOTS x COMB_NMAX elements, grown in chunks
    bool combine = true;  // tuning key combine

    ~NttCtx() {
        for (auto& l : lanes)
            if (l.st) (void)hipStreamDestroy(l.st);
        if (stream) (void)hipStreamDestroy(stream);
    }
    void ensure(size_t n) {
        if (n <= d_a.cap && n <= d_b.cap) return;
        kzgamd::drop_all(d_a, d_b);
        d_a.ensure(n);
        d_b.ensure(n);
    }
};

namespace kzgamd {
// ntt.hip: what kzgamd_ntt_new_ex calls once the configuration is resolved (config.h); NULL on failure
void* ntt_create(unsigned scale, const Options& opt);
// fftg1.hip: G1 transforms of device-resident g1::Xyzz data, see there
void* fftg1_device(NttCtx* ctx, void* data_xyzz, void* scratch_xyzz, size_t n, size_t nbatch, int inverse, hipStream_t st,
                   bool scale_inverse = true);
// The same (never scaled) with per-lane tables of the caller's — 9 * n * nbatch g1::Xyzz — instead of the handle's:
// callers with tables of their own may run beside each other and beside fft_g1 on one handle (generic FK20, fk20.hip).
void* fftg1_device_tab(NttCtx* ctx, void* data_xyzz, void* scratch_xyzz, size_t n, size_t nbatch, int inverse, hipStream_t st,
                       void* tab_xyzz);
// fftg1.hip: out[g] = sum_{i < group} scalars[g * group + i] * bases[(g * group + i) % nbase], g < nprod / group — the
// pointwise products of FK20, the scalars read per product from device memory, already split (one RootSplit each).
// prod: nprod g1::Xyzz of workspace (unused when group == 1), tab: 18 * nprod g1::Xyzz; group: a power of two.  Zero
// scalars and identity bases give the identity.  Enqueued on `st`, nothing synchronised.
void g1_varmul_sum_device(NttCtx* ctx, void* out_xyzz, void* prod_xyzz, void* tab_xyzz, const void* bases_xyzz, size_t nbase,
                          const RootSplit* d_scalars, size_t nprod, size_t group, hipStream_t st);
// fftg1.hip: blst Jacobian <-> g1::Xyzz for `count` device-resident points, natural order
void g1_jacobian_to_xyzz(void* d_xyzz, const void* d_p1, size_t count, hipStream_t st);
void g1_xyzz_to_jacobian(void* d_p1, const void* d_xyzz, size_t count, hipStream_t st);
}  // namespace kzgamd
