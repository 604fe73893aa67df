// Shared between kzg.hip (quotients by X^n - x^n) and poly.hip (Poly::eval): the first-order recurrence
// H_m = S_m + C H_{m+1} over the lanes of a wave, and the table of powers it runs on.
//
// A sequence is cut into chunks of CHUNK consecutive steps, a lane per chunk.  The lane runs its chunk from a zero
// carry (S_m); the true value at the base of chunk m is H_m = S_m + C H_{m+1}, C = c^CHUNK.  scan_suffix solves that
// inside a group of gw lanes of a wave (gw a power of two <= 64) by a log-step suffix scan with the powers C^(2^k);
// waves are chained through one summary each with the powers of C^64, which are the same table from entry 7 on.
// Wave-local exchange only: nothing here needs a workgroup barrier.
//
// Everything sits in an anonymous namespace: each file that includes this header gets its own copy of k_kzg_pows.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ff.hip.h"
#include "fr29.hip.h"

namespace {

constexpr int CHUNK = 16;                   // consecutive steps of a sequence per lane of the chunked form
constexpr int PW = 16;                      // per x: c, then C^(2^k), k = 0 .. 11, C = c^CHUNK (C^64 and its powers chain the waves)
constexpr int NPOW = 12;

__device__ __forceinline__ ff::Fr fr_mul(const ff::Fr& a, const ff::Fr& b) { return fr29::mul_blst(a, b); }

// a^e for a small public exponent
__device__ __forceinline__ ff::Fr fr_pow(const ff::Fr& a, size_t e) {
    ff::Fr r = ff::Fr::one(), b = a;
    while (e) {
        if (e & 1) r = fr_mul(r, b);
        e >>= 1;
        if (e) b = fr_mul(b, b);
    }
    return r;
}

__device__ __forceinline__ ff::Fr shfl_down(const ff::Fr& a, int d) {
    ff::Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = __shfl_down(a.v[i], d, 64);
    return r;
}

// suffix scan over a group of gw lanes: lane lg of the group returns sum_{d >= 0, lg + d < gw} C^d S_{lg + d}, given its
// own S and pw[k] = C^(2^k), k < log2(gw).  Every lane of the wave must call it (lanes without work carry zeros).
__device__ __forceinline__ ff::Fr scan_suffix(const ff::Fr& S, ff::u32 lg, ff::u32 gw, const ff::Fr* __restrict__ pw) {
    ff::Fr H = S;
    for (ff::u32 k = 0; ((ff::u32)1 << k) < gw; ++k) {
        const ff::Fr up = shfl_down(H, 1 << k);
        if (lg + ((ff::u32)1 << k) < gw) H = ff::add(H, fr_mul(pw[k], up));
    }
    return H;
}

// per x: pw[0] = c = x^n, pw[1 + k] = (c^CHUNK)^(2^k), k < NPOW
__global__ void __launch_bounds__(64) k_kzg_pows(ff::Fr* __restrict__ pw, const ff::Fr* __restrict__ xs, size_t n, size_t nx) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nx) return;
    ff::Fr c = xs[t];
    for (size_t m = 1; m < n; m <<= 1) c = fr_mul(c, c);
    pw[t * PW] = c;
    ff::Fr C = fr_pow(c, CHUNK);
    for (int k = 0; k < NPOW; ++k) {
        pw[t * PW + 1 + k] = C;
        C = fr_mul(C, C);
    }
}

}  // namespace
