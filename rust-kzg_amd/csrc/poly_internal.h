// Shared between poly.hip (Poly<Fr>) and zeropoly.hip (ZeroPoly, PolyRecover): the context object behind the opaque
// handle of kzgamd_poly_new(), its workspace buffers and the wave-local exchange of field elements; the frame every call
// runs in (lock, device, stream, one synchronisation) is host_call.h's.  Nothing here launches a kernel of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../include/kzg_mi355x.h"
#include "device_guard.h"
#include "ff.hip.h"
#include "host_call.h"
#include "ntt_internal.h"

namespace kzgamd_poly {

using ff::Fr;
using ff::u32;

__device__ __forceinline__ Fr shfl_xor(const Fr& a, int m) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = __shfl_xor(a.v[i], m, 64);
    return r;
}
__device__ __forceinline__ Fr shfl_idx(const Fr& a, int lane) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = __shfl(a.v[i], lane, 64);
    return r;
}
__device__ __forceinline__ Fr shfl_up(const Fr& a, int d) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = __shfl_up(a.v[i], d, 64);
    return r;
}

using kzgamd::blocks;
using kzgamd::DevBuf;
using kzgamd::next_pow2;
using kzgamd::run_call;

struct PolyCtx {
    NttCtx* ntt = nullptr;
    int device = 0;
    std::mutex mu;
    hipStream_t st = nullptr;
    // workspace, grown as calls need it: operands, inverse, result, the two transform buffers, eval's points and sums
    DevBuf a, b, c, out, f, g, xs, pw, sums, flag;
    // zeropoly.hip: the roots of unity in Montgomery form (W + 1 of them, copied on the first call that needs them),
    // the root indices and the plan tables of a call, the low coefficients of the monic products, recovery's mask
    DevBuf roots, idx, tab, zc, mask;
    bool roots_ready = false;

    std::vector<const DevBuf*> bufs() const { return {&a, &b, &c, &out, &f, &g, &xs, &pw, &sums, &flag, &roots, &idx, &tab, &zc, &mask}; }
    ~PolyCtx() {
        if (st) (void)hipStreamDestroy(st);
    }
};

inline size_t min_sz(size_t a, size_t b) { return a < b ? a : b; }

inline void ntt_on_stream(PolyCtx* pc, Fr* out, const Fr* in, size_t n, size_t nbatch, int inverse) {
    if (kzgamd_ntt_fr_device(pc->ntt, out, in, n, nbatch, inverse, pc->st) != 0) throw kzgamd::DevErr{hipErrorUnknown};
}

// polynomials per slice: the workspace of a slice stays within a share of the free HBM
inline size_t slice_of(PolyCtx* pc, size_t npoly, size_t bytes_per_poly) {
    size_t free_b = 0, total_b = 0, held = 0;
    DEV_TRY(hipMemGetInfo(&free_b, &total_b));
    for (const DevBuf* d : pc->bufs()) held += d->cap;
    size_t per = (free_b + held) / 8 / (bytes_per_poly ? bytes_per_poly : 1);
    if (per == 0) per = 1;
    return per < npoly ? per : npoly;
}

inline void upload(PolyCtx* pc, void* dst, const void* src, size_t bytes) {
    DEV_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, pc->st));
}
inline void download(PolyCtx* pc, void* dst, const void* src, size_t bytes) {
    DEV_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, pc->st));
}

}  // namespace kzgamd_poly
