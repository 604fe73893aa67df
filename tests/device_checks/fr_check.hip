// Test-only harness for the Fr arithmetic of the NTT kernels (fr29.hip.h) and the lane scan of frscan.hip.h.  Never
// linked into the product; includes only headers of rust-kzg_amd/csrc and needs no library.  tests/test_fr_arith_gpu.py
// builds and runs it for the device, tests/test_fr_device_cases_cpu.py cross-compiles it and runs its host form;
// tests/fr29_cases.py holds the cases and the checkers.
//
// stdin:  one case per line:  <op> <nin hex words>      (nin fixed per op, table below)
// stdout: one line of nout hex words per case, in the order of the input
// Device form: all cases of an op run in ONE kernel launch, one case per lane, 64 different cases in a wave.  Case i of
// the op goes to lane (l' - 7 w) mod 64 of wave w, i = l' * nwaves + w: neighbours in the case list (the generator puts
// the edge cases first) land in different waves, on lanes that rotate from wave to wave.  `scan` is one wave per case.
// Host form (-DFR_CHECK_HOST, any C++17 compiler, no HIP): the same run_case() in a loop; no `scan`.
// The output buffer is filled with SENTINEL before the launch: a word an op does not write stays that.
//
// -DFR_CHECK_UNCHAINED   mul_signed / mul_signed2 without the opaque accumulator chain (CHAIN = false)
// -DFR_CHECK_PLANT_ERROR adds 1 to output word 3 of case 1 of every op (lane 37's word 3 for `scan`) after the code
//                        under test has run: the checkers must see it.
#if !defined(FR_CHECK_HOST)
#include <hip/hip_runtime.h>
#endif

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fr29.hip.h"
#if !defined(FR_CHECK_HOST)
#include "frscan.hip.h"
#endif

using ff::u32;
using fr29::Fe;

namespace {
constexpr u32 SENTINEL = 0xA5A5A5A5u;
#if defined(FR_CHECK_UNCHAINED)
constexpr bool CHAINED = false;
#else
constexpr bool CHAINED = true;
#endif

enum Op { OP_ROUND, OP_MSIG, OP_BFS, OP_BFL, OP_BFL8, OP_REDL, OP_FIN, OP_MUL, OP_MSIG2, OP_ROUND_UNIT, OP_TWIST, OP_PACK,
          OP_UNPACK, OP_UNPACK_SHL5, OP_MULB, OP_SCAN, NOPS };
struct OpInfo {
    const char* name;
    int nin, nout;
};
const OpInfo OPS[NOPS] = {{"round", 72, 36}, {"msig", 18, 9}, {"bfs", 18, 18}, {"bfl", 18, 18}, {"bfl8", 18, 18},
                          {"redl", 9, 8}, {"fin", 18, 8}, {"mul", 18, 9}, {"msig2", 36, 18}, {"round_unit", 41, 36},
                          {"twist", 18, 9}, {"pack", 9, 8}, {"unpack", 8, 9}, {"unpack_shl5", 8, 9}, {"mulb", 16, 8},
                          {"scan", 64 * 8 + 1 + 6 * 8, 64 * 8}};

FF_HD Fe ld_fe(const u32* w) {
    Fe a;
#pragma unroll
    for (int i = 0; i < fr29::L; ++i) a.v[i] = w[i];
    return a;
}
FF_HD ff::Fr ld_fr(const u32* w) {
    ff::Fr a;
#pragma unroll
    for (int i = 0; i < 8; ++i) a.v[i] = w[i];
    return a;
}
FF_HD void st(u32* w, const Fe& a) {
#pragma unroll
    for (int i = 0; i < fr29::L; ++i) w[i] = a.v[i];
}
FF_HD void st(u32* w, const ff::Fr& a) {
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = a.v[i];
}
// ntt.hip's KZG_BF
FF_HD void bf(Fe& x, Fe& y, const Fe& w) {
    const Fe t = fr29::mul_signed<CHAINED>(y, w);
    fr29::butterfly_signed(x, y, t);
}

// one case of one op: the calls are the ones of ntt.hip's ntt_round, in its order
FF_HD void run_case(int op, const u32* in, u32* out) {
    switch (op) {
    case OP_ROUND: {  // a round that is not a transform's first: KZG_BF x 4, then one norm each
        Fe e[4], w[4];
        for (int k = 0; k < 4; ++k) e[k] = ld_fe(in + 9 * k);
        for (int k = 0; k < 4; ++k) w[k] = ld_fe(in + 36 + 9 * k);
        bf(e[0], e[1], w[0]);
        bf(e[2], e[3], w[1]);
        bf(e[0], e[2], w[2]);
        bf(e[1], e[3], w[3]);
        for (int k = 0; k < 4; ++k) {
            fr29::norm(e[k]);
            st(out + 9 * k, e[k]);
        }
        break;
    }
    case OP_ROUND_UNIT: {  // a transform's first round: KZG_BF1 x 2, KZG_BF1N(0, 2), KZG_BF(1, 3, w), then one norm each
        Fe e[4];
        for (int k = 0; k < 4; ++k) e[k] = fr29::unpack(ld_fr(in + 8 * k));
        const Fe w = ld_fe(in + 32);
        {
            const Fe y = e[1];
            fr29::butterfly_lazy(e[0], e[1], y);
        }
        {
            const Fe y = e[3];
            fr29::butterfly_lazy(e[2], e[3], y);
        }
        {
            Fe y = e[2];
            fr29::norm(y);
            fr29::butterfly_lazy8(e[0], e[2], y);
        }
        bf(e[1], e[3], w);
        for (int k = 0; k < 4; ++k) {
            fr29::norm(e[k]);
            st(out + 9 * k, e[k]);
        }
        break;
    }
    case OP_MSIG: st(out, fr29::mul_signed<CHAINED>(ld_fe(in), ld_fe(in + 9))); break;
    case OP_MSIG2: {
        Fe r0, r1;
        fr29::mul_signed2<CHAINED>(r0, r1, ld_fe(in), ld_fe(in + 9), ld_fe(in + 18), ld_fe(in + 27));
        st(out, r0);
        st(out + 9, r1);
        break;
    }
    case OP_BFS:
    case OP_BFL:
    case OP_BFL8: {
        Fe x = ld_fe(in), y;
        const Fe t = ld_fe(in + 9);
        if (op == OP_BFS) fr29::butterfly_signed(x, y, t);
        else if (op == OP_BFL) fr29::butterfly_lazy(x, y, t);
        else fr29::butterfly_lazy8(x, y, t);
        st(out, x);
        st(out + 9, y);
        break;
    }
    case OP_REDL: st(out, fr29::reduce_lazy(ld_fe(in))); break;
    case OP_FIN: st(out, fr29::finish(ld_fe(in), ld_fe(in + 9))); break;
    case OP_MUL: st(out, fr29::mul(ld_fe(in), ld_fe(in + 9))); break;
    case OP_TWIST: {  // ntt_round's twist of the DAS extension
        Fe e = fr29::mul_signed<CHAINED>(ld_fe(in), ld_fe(in + 9));
#pragma unroll
        for (int l = 0; l < fr29::L; ++l) e.v[l] += fr29::rl(l);
        fr29::norm(e);
        st(out, e);
        break;
    }
    case OP_PACK: st(out, fr29::pack(ld_fe(in))); break;
    case OP_UNPACK: st(out, fr29::unpack(ld_fr(in))); break;
    case OP_UNPACK_SHL5: st(out, fr29::unpack_shl5(ld_fr(in))); break;
    case OP_MULB: st(out, fr29::mul_blst(ld_fr(in), ld_fr(in + 8))); break;
    default: break;
    }
}

#if defined(FR_CHECK_PLANT_ERROR)
constexpr bool PLANT = true;
#else
constexpr bool PLANT = false;
#endif

#if !defined(FR_CHECK_HOST)
// the case a thread runs (see the head of the file); >= n: none
__device__ __forceinline__ size_t case_of_thread(u32 wave, u32 lane, u32 nwaves) { return (size_t)((lane + 7u * wave) & 63u) * nwaves + wave; }

__global__ void __launch_bounds__(64) k_lane_cases(int op, const u32* __restrict__ in_all, u32* __restrict__ out_all, int nin, int nout, u32 n) {
    const size_t i = case_of_thread(blockIdx.x, threadIdx.x, gridDim.x);
    if (i >= n) return;
    u32* out = out_all + i * nout;
    run_case(op, in_all + i * nin, out);
    if (PLANT && i == 1) out[3] += 1;
}

// one wave per case: lanes' S (64 x 8 words), the group width, C^(2^k) for k < 6
__global__ void __launch_bounds__(64) k_scan(const u32* __restrict__ in_all, u32* __restrict__ out_all, int nin, int nout) {
    const u32 lane = threadIdx.x;
    const u32* in = in_all + (size_t)blockIdx.x * nin;
    u32* out = out_all + (size_t)blockIdx.x * nout;
    const u32 gw = in[64 * 8];
    ff::Fr pw[6];
    for (int k = 0; k < 6; ++k) pw[k] = ld_fr(in + 64 * 8 + 1 + 8 * k);
    const ff::Fr H = scan_suffix(ld_fr(in + 8 * lane), lane & (gw - 1), gw, pw);
    st(out + 8 * lane, H);
    if (PLANT && blockIdx.x == 1 && lane == 37) out[8 * lane + 3] += 1;
}

#define HIP_TRY(X)                                                                   \
    do {                                                                             \
        hipError_t e_ = (X);                                                         \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "HIP error %s at %s\n", hipGetErrorString(e_), #X);      \
            printf("error\n");                                                       \
            exit(3);                                                                 \
        }                                                                            \
    } while (0)

void run_op(int op, const std::vector<u32>& in, std::vector<u32>& out, size_t n) {
    const int nin = OPS[op].nin, nout = OPS[op].nout;
    u32 *d_in = nullptr, *d_out = nullptr;
    HIP_TRY(hipMalloc(&d_in, in.size() * sizeof(u32)));
    HIP_TRY(hipMalloc(&d_out, out.size() * sizeof(u32)));
    HIP_TRY(hipMemcpy(d_in, in.data(), in.size() * sizeof(u32), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_out, out.data(), out.size() * sizeof(u32), hipMemcpyHostToDevice));
    if (op == OP_SCAN) hipLaunchKernelGGL(k_scan, dim3((unsigned)n), dim3(64), 0, 0, d_in, d_out, nin, nout);
    else hipLaunchKernelGGL(k_lane_cases, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, op, d_in, d_out, nin, nout, (u32)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out.data(), d_out, out.size() * sizeof(u32), hipMemcpyDeviceToHost));
    HIP_TRY(hipFree(d_in));
    HIP_TRY(hipFree(d_out));
}
#else
void run_op(int op, const std::vector<u32>& in, std::vector<u32>& out, size_t n) {
    const int nin = OPS[op].nin, nout = OPS[op].nout;
    if (op == OP_SCAN) {
        printf("error: scan is device-only\n");
        exit(2);
    }
    for (size_t i = 0; i < n; ++i) {
        run_case(op, in.data() + i * nin, out.data() + i * nout);
        if (PLANT && i == 1) out[i * nout + 3] += 1;
    }
}
#endif
}  // namespace

int main() {
    std::vector<u32> in[NOPS], out[NOPS];
    std::vector<std::pair<int, size_t>> order;  // (op, index among the op's cases) per input line
    char name[32];
    while (scanf("%31s", name) == 1) {
        int op = -1;
        for (int k = 0; k < NOPS; ++k)
            if (!strcmp(name, OPS[k].name)) op = k;
        if (op < 0) {
            printf("error: unknown op %s\n", name);
            return 1;
        }
        for (int k = 0; k < OPS[op].nin; ++k) {
            u32 w = 0;
            if (scanf("%x", &w) != 1) {
                printf("error: short input for %s\n", name);
                return 1;
            }
            in[op].push_back(w);
        }
        order.push_back({op, in[op].size() / OPS[op].nin - 1});
    }
    for (int op = 0; op < NOPS; ++op) {
        const size_t n = in[op].size() / OPS[op].nin;
        if (!n) continue;
        out[op].assign(n * OPS[op].nout, SENTINEL);
        run_op(op, in[op], out[op], n);
    }
    for (const auto& oi : order) {
        const int nout = OPS[oi.first].nout;
        const u32* o = out[oi.first].data() + oi.second * nout;
        std::string line;
        char buf[16];
        for (int k = 0; k < nout; ++k) {
            snprintf(buf, sizeof buf, "%x ", o[k]);
            line += buf;
        }
        puts(line.c_str());
    }
    return 0;
}
