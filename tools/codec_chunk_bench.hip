// How many points should a lane of k_g1_jac_out (codec.hip) take?  g1io::jac_chunk_out with chunks of 1, 4, 8 and 16
// Jacobian points per lane (one inversion per lane), compress and to-affine, at 2^15 ... 2^20 points: kernel time by
// events, the median of 10 launches after a warm-up, one JSON line per (points, chunk).  The inputs are random canonical
// coordinates (the arithmetic does not care whether they are on the curve) with every 16th point the identity.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/codec_chunk_bench.hip -o tools/codec_chunk_bench
//   tools/codec_chunk_bench >> profiles/codec_chunk.jsonl
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../rust-kzg_amd/csrc/g1_io.hip.h"

#define CHECK(x)                                                                   \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                \
            return 1;                                                              \
        }                                                                          \
    } while (0)

template <int CH, bool AFFINE>
__global__ void __launch_bounds__(64) k_out(void* __restrict__ out, const ff::Fp* __restrict__ in, size_t n) {
    const size_t at = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * CH;
    if (at >= n) return;
    const int m = n - at < (size_t)CH ? (int)(n - at) : CH;
    g1io::jac_chunk_out<CH, AFFINE>((unsigned char*)out + at * (AFFINE ? 96 : 48), in + 3 * at, m);
}

template <int CH, bool AFFINE>
int run(void* d_out, const ff::Fp* d_in, size_t n, float* median_ms) {
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    const unsigned lanes = (unsigned)((n + CH - 1) / CH), grid = (lanes + 63) / 64;
    std::vector<float> ts;
    for (int rep = 0; rep < 11; ++rep) {
        CHECK(hipEventRecord(a, 0));
        hipLaunchKernelGGL((k_out<CH, AFFINE>), dim3(grid), dim3(64), 0, 0, d_out, d_in, n);
        CHECK(hipEventRecord(b, 0));
        CHECK(hipEventSynchronize(b));
        CHECK(hipGetLastError());
        float ms;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (rep) ts.push_back(ms);
    }
    std::sort(ts.begin(), ts.end());
    *median_ms = ts[ts.size() / 2];
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
    return 0;
}

int main() {
    const size_t sizes[6] = {(size_t)1 << 15, (size_t)1 << 16, (size_t)1 << 17, (size_t)1 << 18, (size_t)1 << 19, (size_t)1 << 20};
    const size_t nmax = sizes[5];
    std::vector<ff::Fp> h(3 * nmax);
    unsigned long long s = 0x9e3779b97f4a7c15ull;
    for (size_t i = 0; i < 3 * nmax; ++i) {
        for (int k = 0; k < 12; ++k) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            h[i].v[k] = (ff::u32)(s >> 32);
        }
        h[i].v[11] &= 0x0fffffffu;  // below p
        if (i % 3 == 2 && (i / 3) % 16 == 5)
            for (int k = 0; k < 12; ++k) h[i].v[k] = 0;  // Z = 0: the identity
    }
    ff::Fp* d_in;
    void* d_out;
    CHECK(hipMalloc(&d_in, 3 * nmax * sizeof(ff::Fp)));
    CHECK(hipMalloc(&d_out, nmax * 96));
    CHECK(hipMemcpy(d_in, h.data(), 3 * nmax * sizeof(ff::Fp), hipMemcpyHostToDevice));
    for (size_t n : sizes) {
        float c[4], a[4];
        if (run<1, false>(d_out, d_in, n, &c[0]) || run<4, false>(d_out, d_in, n, &c[1]) || run<8, false>(d_out, d_in, n, &c[2]) ||
            run<16, false>(d_out, d_in, n, &c[3]) || run<1, true>(d_out, d_in, n, &a[0]) || run<4, true>(d_out, d_in, n, &a[1]) ||
            run<8, true>(d_out, d_in, n, &a[2]) || run<16, true>(d_out, d_in, n, &a[3]))
            return 1;
        const int ch[4] = {1, 4, 8, 16};
        for (int i = 0; i < 4; ++i)
            printf("{\"points\": %zu, \"chunk\": %d, \"compress_kernel_ms\": %.4f, \"to_affine_kernel_ms\": %.4f}\n", n, ch[i], c[i], a[i]);
    }
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    return 0;
}
