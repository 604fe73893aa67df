// The inputs of a combined batch (combine.h) stay where their callers staged them, in page-locked, mapped slots: one
// kernel fetches them over PCIe into the batch's contiguous device buffer, and one writes results back, instead of one
// copy operation per request on the stream.  Included by msm.hip and ntt.hip; internal linkage in each.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct SlotPtrs {
    static constexpr size_t MAX = 32;  // the largest batch of either user: each asserts it against its own constant
    uint4* p[MAX];
};
// request j of nreq: `per` 16-byte words
static __global__ void __launch_bounds__(256) k_slots_gather(uint4* __restrict__ dst, SlotPtrs slots, size_t per, size_t nreq) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nreq * per) dst[t] = slots.p[t / per][t % per];
}
[[maybe_unused]] static __global__ void __launch_bounds__(256) k_slots_scatter(SlotPtrs slots, const uint4* __restrict__ src, size_t per, size_t nreq) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nreq * per) slots.p[t / per][t % per] = src[t];
}
