// G2 linear combinations on the GPU (setupcheck.hip), the form other code of the library uses: device-resident inputs,
// stream-ordered, no synchronisation; and the powers kernel of groupmul.hip for callers outside that file.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ff.hip.h"

namespace kzgamd {

// d_out[i] = c * s^(start + i), i < n (Montgomery blst_fr in and out), enqueued on `st` (groupmul.hip: k_fr_powers)
void fr_powers_enqueue(ff::Fr* d_out, const ff::Fr& s, const ff::Fr& c, size_t start, size_t n, hipStream_t st);

namespace g2lc_gpu {
// bytes of workspace one run over up to n points needs
size_t work_bytes(size_t n);
// *d_out (a blst_p2: Jacobian, canonical, all-zero for the identity) = sum_i d_scalars[i] * d_points[i], i < n, n >= 1:
// blst_p2 points (canonical coordinates, any Z, Z == 0 the identity) and Montgomery blst_fr scalars, everything
// device-resident, enqueued on `st` of the current device.  d_work: work_bytes(n) bytes, busy until the stream has
// passed the run.  The caller collects launch errors (hipGetLastError).
void lincomb_enqueue(void* d_out, const void* d_points, const void* d_scalars, size_t n, void* d_work, hipStream_t st);
}  // namespace g2lc_gpu

}  // namespace kzgamd
