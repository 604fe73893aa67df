// Fixed-base batched scalar multiplication in G1 and in G2, and the trusted setups built from it:
//     out[i] = k_i * B                      kzgamd_g1_mul_batch / kzgamd_g2_mul_batch   (G1Mul::mul / G2Mul::mul, batched)
//     [s^i]G1, their Lagrange form, [s^j]G2 kzgamd_generate_trusted_setup               (blst/src/utils.rs:16-37)
//
// One table per call and group: T[k][j - 1] = j * 2^(8k) * B as affine points, k < 32 windows of 8 bits, j = 1 .. 128.
// A scalar below r is recoded into 32 signed digits d_k in [-128, 128] (a digit above 128 becomes d - 256 and carries
// one into the next window; the top window of a scalar below r < 0x74 * 2^248 holds at most 0x73 + 1, so nothing
// carries out), and a lane adds T[k][|d_k| - 1] or its negative for every non-zero digit: at most 32 mixed additions
// per output, no doubling.  Signed digits halve the table (and the serial chain that builds it) against unsigned ones;
// 8 bits keep the table of either group below 1 MB, which stays in the L2 of every XCD while all lanes gather from it.
// Every addition of the walk takes the complete form (g1::chain_add; g2::madd_complete), so P + P and P - P cost a
// branch that is never taken for a base of order r (profiles/NOTES.md, section 35, has the argument) but is right for
// any base.
//
// The table is built on the device in two launches: a lane per window doubles B 8k times, normalises, and adds its
// way up the 128 multiples; a lane per entry then converts to affine with an inversion of its own.  The tables of the
// two generators are built once per device and kept; a caller's base gets a table for the call.
//
// Powers of the secret are computed on the device (k_fr_powers: a lane starts from c * s^(16 t) by square-and-multiply
// and multiplies on 16 times), so a setup uploads one scalar.  The Lagrange form is the inverse G1 transform of the
// device-resident points [s^i / n]G (the n^-1 of the inverse transform folded into the scalars) through
// kzgamd::fftg1_device_tab with tables of this call's own: nothing goes through the host, and calls may run beside
// each other and beside fft_g1 on one NTT handle.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/kzg_mi355x.h"
#include "config.h"
#include "device_guard.h"
#include "ff.hip.h"
#include "fr29.hip.h"
#include "g1_28.hip.h"
#include "g1_io.hip.h"
#include "g2_28.hip.h"
#include "g2_bucket.hip.h"
#include "host_call.h"
#include "host_fp64.h"
#include "host_g1.h"
#include "host_pairing.h"
#include "ntt_internal.h"
#include "setupcheck_internal.h"

using ff::Fr;
using ff::u32;
using ff::u64;
using g1::Xyzz;
using kzgamd::blocks;
using kzgamd::ScopedBuf;

namespace {

constexpr int WBITS = 8;                  // window width
constexpr int NWIN = 32;                  // windows of a 256-bit scalar
constexpr int HALF = 1 << (WBITS - 1);    // table entries per window: the multiples 1 .. 128
constexpr int NTAB = NWIN * HALF;         // entries of a table
constexpr int POW_CHUNK = 16;             // consecutive powers per lane of k_fr_powers
constexpr size_t SLICE_DEFAULT = (size_t)1 << 18;  // outputs per slice: 8 MB of scalars, 58 MB of XYZZ, 75 MB of blst_p2
constexpr size_t SLICE_MIN = 64;
constexpr size_t FFT_TAB = 9;             // g1::Xyzz of table per point that fftg1_device_tab asks for (ntt_internal.h)

// out[i] = c * s^(start + i), i < n; blst Montgomery form in and out
__global__ void __launch_bounds__(256) k_fr_powers(Fr* __restrict__ out, Fr s, Fr c, u64 start, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t at = t * POW_CHUNK;
    if (at >= n) return;
    Fr acc = c, b = s;
    for (u64 e = start + at; e; e >>= 1) {
        if (e & 1) acc = fr29::mul_blst(acc, b);
        if (e >> 1) b = fr29::mul_blst(b, b);
    }
    const size_t end = n - at < (size_t)POW_CHUNK ? n - at : (size_t)POW_CHUNK;
    for (size_t i = 0; i < end; ++i) {
        out[at + i] = acc;
        if (i + 1 < end) acc = fr29::mul_blst(acc, s);
    }
}

// digit k of the signed base-256 recoding: g2_bucket.hip.h has it, for this file and for g2msm.hip
using g2b::signed_digit;
static_assert(WBITS == g2b::WBITS && NWIN == g2b::NWIN && HALF == g2b::HALF, "one recoding");

// ---------------------------------------------------------------- G1
// lane k < 32: tmp[k][j - 1] = j * 2^(8k) * B, j = 1 .. 128, as XYZZ (entry 0 normalised: ZZ = ZZZ = 1).
// B is affine, canonical, of order r: no entry is infinity (j * 2^(8k) is no multiple of r).
__global__ void __launch_bounds__(64) k_g1_tab_chain(Xyzz* __restrict__ tmp, g1::AffPt base) {
    const int k = threadIdx.x;
    if (k >= NWIN) return;
    Xyzz acc;
    g1::set_affine(acc, base.x, base.y);
    g1::dbl_k(acc, WBITS * k);
    const fp28::Fe zi = g1io::inverse(fp28::mul(acc.zz, acc.zzz));
    const fp28::Fe x = fp28::canon(fp28::mul(acc.x, fp28::mul(zi, acc.zzz)));
    const fp28::Fe y = fp28::canon(fp28::mul(acc.y, fp28::mul(zi, acc.zz)));
    g1::set_affine(acc, x, y);
    tmp[k * HALF] = acc;
    for (int j = 1; j < HALF; ++j) {
        g1::madd(acc, x, y);  // complete: the first step is P + P
        tmp[k * HALF + j] = acc;
    }
}
__global__ void __launch_bounds__(64) k_g1_tab_affine(g1::AffPt* __restrict__ tab, const Xyzz* __restrict__ tmp) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= NTAB) return;
    const Xyzz p = tmp[t];
    g1::AffPt a;  // never infinity: see k_g1_tab_chain
    a.pad[0] = a.pad[1] = a.pad[2] = 0;
    const fp28::Fe zi = g1io::inverse(fp28::mul(p.zz, p.zzz));
    a.x = fp28::canon(fp28::mul(p.x, fp28::mul(zi, p.zzz)));
    a.y = fp28::canon(fp28::mul(p.y, fp28::mul(zi, p.zz)));
    a.flags = 0;
    tab[t] = a;
}
// out[i] = scalars[i] * B as XYZZ (the bounds of g1_28.hip.h: what g1::chain_add leaves); scalars in Montgomery form
__global__ void __launch_bounds__(256) k_g1_mul(Xyzz* __restrict__ out, const Fr* __restrict__ scalars,
                                                const g1::AffPt* __restrict__ tab, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fr k = ff::from_mont(scalars[i]);
    Xyzz acc;
    g1::set_inf(acc);
    u32 st = g1::CHAIN_EMPTY, carry = 0;
#pragma unroll 1
    for (int w = 0; w < NWIN; ++w) {
        u32 neg;
        const u32 d = signed_digit(k, w, carry, neg);
        if (d == 0) continue;
        const g1::AffPt* e = tab + w * HALF + (d - 1);  // no entry is infinity: the base is tested to be of order r
        const fp28::Fe x = e->x, y = e->y;
        g1::chain_add(acc, st, x, y, neg);
    }
    out[i] = acc;
}

// ---------------------------------------------------------------- G2
// as k_g1_tab_chain.  A G2 base is the caller's responsibility, and the table of one outside the subgroup is still
// right: the group E'(Fp2) has odd order (r times an odd cofactor), so no doubling of a point other than infinity
// gives infinity and every window has a base; the multiples j * 2^(8k) * B may be infinity (j a multiple of the order
// of B), which the complete addition of the chain takes, k_g2_tab_affine flags, and the walk steps over
// (g2::madd_tab).  tests/test_group_mul_gpu.py runs a base of order 13 and one of full order.
// (Two kernels, the doublings apart from the chain: as one, the compiler kept 332 bytes of the lane in scratch.)
__global__ void __launch_bounds__(64) k_g2_tab_base(g2::AffPt* __restrict__ bases, g2::AffPt base) {
    const int k = threadIdx.x;
    if (k >= NWIN) return;
    g2::Jac acc;
    g2::set_affine(acc, base.x, base.y);
#pragma unroll 1
    for (int i = 0; i < WBITS * k; ++i) g2::dbl(acc);
    g2::AffPt a;
    g2::to_affine(a, acc);
    bases[k] = a;
}
__global__ void __launch_bounds__(64) k_g2_tab_chain(g2::Jac* __restrict__ tmp, const g2::AffPt* __restrict__ bases) {
    const int k = threadIdx.x;
    if (k >= NWIN) return;
    const g2::AffPt a = bases[k];
    g2::Jac acc;
    g2::set_affine(acc, a.x, a.y);
    tmp[k * HALF] = acc;
    for (int j = 1; j < HALF; ++j) {
        g2::madd_complete(acc, a.x, a.y);
        tmp[k * HALF + j] = acc;
    }
}
__global__ void __launch_bounds__(64) k_g2_tab_affine(g2::AffPt* __restrict__ tab, const g2::Jac* __restrict__ tmp) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= NTAB) return;
    g2::AffPt a;
    g2::to_affine(a, tmp[t]);
    tab[t] = a;
}
// out[i] = scalars[i] * B in the blst_p2 layout (six Fp per point, canonical; infinity all-zero)
__global__ void __launch_bounds__(64) k_g2_mul(ff::Fp* __restrict__ out, const Fr* __restrict__ scalars,
                                               const g2::AffPt* __restrict__ tab, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fr k = ff::from_mont(scalars[i]);
    g2::Jac acc;
    g2::set_inf(acc);
    u32 carry = 0;
#pragma unroll 1
    for (int w = 0; w < NWIN; ++w) {
        u32 neg;
        const u32 d = signed_digit(k, w, carry, neg);
        if (d == 0) continue;
        g2::madd_tab(acc, tab[w * HALF + (d - 1)], neg);
    }
    g2::to_blst_jacobian(out + 6 * i, acc);
}

// ---------------------------------------------------------------- host side
namespace hp = kzgamd::pairing;

using Stream = kzgamd::CallStream;

g1::AffPt g1_affpt(const ff::Fp& x, const ff::Fp& y) {  // canonical blst affine coordinates -> table-point form
    g1::AffPt a;
    a.x = fp28::canon(fp28::from_blst(x));
    a.y = fp28::canon(fp28::from_blst(y));
    a.flags = 0;
    a.pad[0] = a.pad[1] = a.pad[2] = 0;
    return a;
}
g2::AffPt g2_affpt(const hp::G2Affine& q) {
    g2::AffPt a;
    a.x = {fp28::canon(fp28::from_blst(q.x.c0)), fp28::canon(fp28::from_blst(q.x.c1))};
    a.y = {fp28::canon(fp28::from_blst(q.y.c0)), fp28::canon(fp28::from_blst(q.y.c1))};
    a.flags = 0;
    a.pad[0] = a.pad[1] = a.pad[2] = 0;
    return a;
}

// the table of `base` on the current device, built on `st` and complete when this returns
void build_g1_table(g1::AffPt* d_tab, const g1::AffPt& base, hipStream_t st) {
    ScopedBuf tmp;
    tmp.alloc((size_t)NTAB * sizeof(Xyzz));
    hipLaunchKernelGGL(k_g1_tab_chain, dim3(1), dim3(64), 0, st, (Xyzz*)tmp.p, base);
    hipLaunchKernelGGL(k_g1_tab_affine, dim3(blocks(NTAB, 64)), dim3(64), 0, st, d_tab, (const Xyzz*)tmp.p);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipStreamSynchronize(st));
}
void build_g2_table(g2::AffPt* d_tab, const g2::AffPt& base, hipStream_t st) {
    ScopedBuf tmp, bases;
    tmp.alloc((size_t)NTAB * sizeof(g2::Jac));
    bases.alloc((size_t)NWIN * sizeof(g2::AffPt));
    hipLaunchKernelGGL(k_g2_tab_base, dim3(1), dim3(64), 0, st, (g2::AffPt*)bases.p, base);
    hipLaunchKernelGGL(k_g2_tab_chain, dim3(1), dim3(64), 0, st, (g2::Jac*)tmp.p, (const g2::AffPt*)bases.p);
    hipLaunchKernelGGL(k_g2_tab_affine, dim3(blocks(NTAB, 64)), dim3(64), 0, st, d_tab, (const g2::Jac*)tmp.p);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipStreamSynchronize(st));
}

// the generators' tables: built at first use on a device, read-only and kept from then on
struct GenTables {
    int device;
    g1::AffPt* g1 = nullptr;
    g2::AffPt* g2 = nullptr;
};
std::mutex g_mu;
std::vector<GenTables> g_gen;

GenTables* gen_entry(int device) {  // under g_mu
    for (GenTables& t : g_gen)
        if (t.device == device) return &t;
    g_gen.push_back(GenTables{device});
    return &g_gen.back();
}
const g1::AffPt* g1_generator_table(int device, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_mu);
    GenTables* t = gen_entry(device);
    if (!t->g1) {
        ScopedBuf tab;
        tab.alloc((size_t)NTAB * sizeof(g1::AffPt));
        ff::Fp x, y;
        kzgamd::host_g1_generator(x, y);
        build_g1_table((g1::AffPt*)tab.p, g1_affpt(x, y), st);
        t->g1 = (g1::AffPt*)tab.p;
        tab.p = nullptr;
    }
    return t->g1;
}
const g2::AffPt* g2_generator_table(int device, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_mu);
    GenTables* t = gen_entry(device);
    if (!t->g2) {
        ScopedBuf tab;
        tab.alloc((size_t)NTAB * sizeof(g2::AffPt));
        build_g2_table((g2::AffPt*)tab.p, g2_affpt(hp::g2_to_affine(hp::g2_generator())), st);
        t->g2 = (g2::AffPt*)tab.p;
        tab.p = nullptr;
    }
    return t->g2;
}

// what a KzgAmdConfig means to these calls: 0, or the call's return code
int read_config(const KzgAmdConfig* cfg, const char* who, int* device, size_t* slice) {
    return kzgamd::read_slice_config(cfg, who, "mul_slice", SLICE_DEFAULT, SLICE_MIN, device, slice);
}

int current_or(int device, hipError_t* e) {
    *e = hipSuccess;
    if (device >= 0) return device;
    int cur = 0;
    *e = hipGetDevice(&cur);
    return cur;
}

// per-call workspace of one slice
struct SliceBufs {
    ScopedBuf sc, xyzz, pts;
    void alloc(size_t slice, bool g1, bool g2) {
        sc.alloc(slice * sizeof(Fr));
        if (g1) xyzz.alloc(slice * sizeof(Xyzz));
        pts.alloc(slice * (g2 ? sizeof(blst_p2) : sizeof(blst_p1)));
    }
};

void enqueue_g1_mul(Xyzz* d_out, const Fr* d_sc, const g1::AffPt* tab, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_g1_mul, dim3(blocks(n, 256)), dim3(256), 0, st, d_out, d_sc, tab, n);
}
void enqueue_g2_mul(void* d_out, const Fr* d_sc, const g2::AffPt* tab, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_g2_mul, dim3(blocks(n, 64)), dim3(64), 0, st, (ff::Fp*)d_out, d_sc, tab, n);
}
void enqueue_powers(Fr* d_out, const Fr& s, const Fr& c, size_t start, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_fr_powers, dim3(blocks((n + POW_CHUNK - 1) / POW_CHUNK, 256)), dim3(256), 0, st, d_out, s, c, (u64)start, n);
}

}  // namespace

void kzgamd::fr_powers_enqueue(Fr* d_out, const Fr& s, const Fr& c, size_t start, size_t n, hipStream_t st) {
    enqueue_powers(d_out, s, c, start, n, st);
}

extern "C" int kzgamd_group_mul_info(size_t* slice_points, int* g1_window_bits, int* g2_window_bits) {
    if (slice_points) *slice_points = SLICE_DEFAULT;
    if (g1_window_bits) *g1_window_bits = WBITS;
    if (g2_window_bits) *g2_window_bits = WBITS;
    return 0;
}

extern "C" int kzgamd_g1_mul_batch(blst_p1* out, const blst_p1* base, const blst_fr* scalars, size_t n, const KzgAmdConfig* cfg) {
    if (n == 0) return 0;
    if (!out || !scalars) return -1;
    int device;
    size_t slice;
    if (int rc = read_config(cfg, "kzgamd_g1_mul_batch", &device, &slice)) return rc;
    g1::AffPt b;
    if (base) {
        ff::Fp x, y;
        if (kzgamd::host_p1_to_affine(base, x, y)) {
            memset(out, 0, n * sizeof(blst_p1));
            return 0;
        }
        if (!kzgamd::host_p1_in_g1(base)) return 3;
        b = g1_affpt(x, y);
    }
    return kzgamd::status_of([&] {
        hipError_t e;
        device = current_or(device, &e);
        DEV_TRY(e);
        kzgamd::DeviceGuard on_device(device);
        DEV_TRY(on_device.err);
        Stream s;
        ScopedBuf own;
        const g1::AffPt* tab;
        if (base) {
            own.alloc((size_t)NTAB * sizeof(g1::AffPt));
            build_g1_table((g1::AffPt*)own.p, b, s.st);
            tab = (const g1::AffPt*)own.p;
        } else {
            tab = g1_generator_table(device, s.st);
        }
        if (slice > n) slice = n;
        SliceBufs w;
        w.alloc(slice, true, false);
        for (size_t at = 0; at < n; at += slice) {
            const size_t cnt = n - at < slice ? n - at : slice;
            DEV_TRY(hipMemcpyAsync(w.sc.p, scalars + at, cnt * sizeof(Fr), hipMemcpyHostToDevice, s.st));
            enqueue_g1_mul((Xyzz*)w.xyzz.p, (const Fr*)w.sc.p, tab, cnt, s.st);
            kzgamd::g1_xyzz_to_jacobian(w.pts.p, w.xyzz.p, cnt, s.st);
            DEV_TRY(hipGetLastError());
            DEV_TRY(hipMemcpyAsync(out + at, w.pts.p, cnt * sizeof(blst_p1), hipMemcpyDeviceToHost, s.st));
            DEV_TRY(hipStreamSynchronize(s.st));
        }
    });
}

extern "C" int kzgamd_g2_mul_batch(blst_p2* out, const blst_p2* base, const blst_fr* scalars, size_t n, const KzgAmdConfig* cfg) {
    if (n == 0) return 0;
    if (!out || !scalars) return -1;
    int device;
    size_t slice;
    if (int rc = read_config(cfg, "kzgamd_g2_mul_batch", &device, &slice)) return rc;
    g2::AffPt b;
    if (base) {
        hp::G2Jac p;
        memcpy(&p, base, sizeof p);
        if (hp::g2_is_inf(p)) {
            memset(out, 0, n * sizeof(blst_p2));
            return 0;
        }
        b = g2_affpt(hp::g2_to_affine(p));
    }
    return kzgamd::status_of([&] {
        hipError_t e;
        device = current_or(device, &e);
        DEV_TRY(e);
        kzgamd::DeviceGuard on_device(device);
        DEV_TRY(on_device.err);
        Stream s;
        ScopedBuf own;
        const g2::AffPt* tab;
        if (base) {
            own.alloc((size_t)NTAB * sizeof(g2::AffPt));
            build_g2_table((g2::AffPt*)own.p, b, s.st);
            tab = (const g2::AffPt*)own.p;
        } else {
            tab = g2_generator_table(device, s.st);
        }
        if (slice > n) slice = n;
        SliceBufs w;
        w.alloc(slice, false, true);
        for (size_t at = 0; at < n; at += slice) {
            const size_t cnt = n - at < slice ? n - at : slice;
            DEV_TRY(hipMemcpyAsync(w.sc.p, scalars + at, cnt * sizeof(Fr), hipMemcpyHostToDevice, s.st));
            enqueue_g2_mul(w.pts.p, (const Fr*)w.sc.p, tab, cnt, s.st);
            DEV_TRY(hipGetLastError());
            DEV_TRY(hipMemcpyAsync(out + at, w.pts.p, cnt * sizeof(blst_p2), hipMemcpyDeviceToHost, s.st));
            DEV_TRY(hipStreamSynchronize(s.st));
        }
    });
}

extern "C" int kzgamd_generate_trusted_setup(void* vntt, blst_p1* g1_monomial, blst_p1* g1_lagrange, blst_p2* g2_monomial,
                                             size_t num_g1, size_t num_g2, const uint8_t secret[32], const KzgAmdConfig* cfg) {
    const bool want_mono = g1_monomial && num_g1, want_lag = g1_lagrange && num_g1, want_g2 = g2_monomial && num_g2;
    if (num_g1 == 0 && num_g2 == 0) return 0;
    if (!want_mono && !want_lag && !want_g2) return 0;
    if (!secret) return -1;
    NttCtx* ntt = (NttCtx*)vntt;
    if (want_lag) {
        if (!ntt || (num_g1 & (num_g1 - 1))) return 1;
        if (num_g1 > ntt->W) return 2;
    }
    int device;
    size_t slice;
    if (int rc = read_config(cfg, "kzgamd_generate_trusted_setup", &device, &slice)) return rc;
    // hash_to_bls_field: the 32 bytes as a big-endian integer mod r, Montgomery form
    Fr s;
    for (int i = 0; i < 8; ++i) {
        const uint8_t* q = secret + (7 - i) * 4;
        s.v[i] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
    }
    s = ff::mul(s, Fr::r2());
    return kzgamd::status_of([&] {
        hipError_t e = hipSuccess;
        device = want_lag ? ntt->device : current_or(device, &e);  // the transform runs where its handle lives
        DEV_TRY(e);
        kzgamd::DeviceGuard on_device(device);
        DEV_TRY(on_device.err);
        Stream st;
        const size_t g1n = want_mono || want_lag ? num_g1 : 0, g2n = want_g2 ? num_g2 : 0;  // of the outputs wanted
        const size_t most = g1n > g2n ? g1n : g2n;
        if (slice > most) slice = most;
        SliceBufs w;
        w.alloc(slice, want_mono, want_g2);  // the Lagrange path writes its XYZZ points where the transform reads them
        const Fr one = Fr::one();
        if (want_mono || want_lag) {
            const g1::AffPt* tab = g1_generator_table(device, st.st);
            if (want_mono) {
                for (size_t at = 0; at < num_g1; at += slice) {
                    const size_t cnt = num_g1 - at < slice ? num_g1 - at : slice;
                    enqueue_powers((Fr*)w.sc.p, s, one, at, cnt, st.st);
                    enqueue_g1_mul((Xyzz*)w.xyzz.p, (const Fr*)w.sc.p, tab, cnt, st.st);
                    kzgamd::g1_xyzz_to_jacobian(w.pts.p, w.xyzz.p, cnt, st.st);
                    DEV_TRY(hipGetLastError());
                    DEV_TRY(hipMemcpyAsync(g1_monomial + at, w.pts.p, cnt * sizeof(blst_p1), hipMemcpyDeviceToHost, st.st));
                    DEV_TRY(hipStreamSynchronize(st.st));
                }
            }
            if (want_lag) {
                // the points [s^i / n]G, device-resident, through the unscaled inverse transform
                ScopedBuf a, b, ftab;
                a.alloc(num_g1 * sizeof(Xyzz));
                b.alloc(num_g1 * sizeof(Xyzz));
                ftab.alloc(FFT_TAB * num_g1 * sizeof(Xyzz));
                Fr nn = Fr::zero();
                nn.v[0] = (u32)num_g1;
                nn.v[1] = (u32)((u64)num_g1 >> 32);
                const Fr inv_n = ff::inverse_bgcd(ff::to_mont(nn));
                for (size_t at = 0; at < num_g1; at += slice) {
                    const size_t cnt = num_g1 - at < slice ? num_g1 - at : slice;
                    enqueue_powers((Fr*)w.sc.p, s, inv_n, at, cnt, st.st);
                    enqueue_g1_mul((Xyzz*)a.p + at, (const Fr*)w.sc.p, tab, cnt, st.st);
                }
                DEV_TRY(hipGetLastError());
                const Xyzz* res = (const Xyzz*)kzgamd::fftg1_device_tab(ntt, a.p, b.p, num_g1, 1, 1, st.st, ftab.p);
                if (!res) throw kzgamd::DevErr{hipErrorOutOfMemory};
                for (size_t at = 0; at < num_g1; at += slice) {
                    const size_t cnt = num_g1 - at < slice ? num_g1 - at : slice;
                    kzgamd::g1_xyzz_to_jacobian(w.pts.p, res + at, cnt, st.st);
                    DEV_TRY(hipGetLastError());
                    DEV_TRY(hipMemcpyAsync(g1_lagrange + at, w.pts.p, cnt * sizeof(blst_p1), hipMemcpyDeviceToHost, st.st));
                    DEV_TRY(hipStreamSynchronize(st.st));
                }
            }
        }
        if (want_g2) {
            const g2::AffPt* tab = g2_generator_table(device, st.st);
            for (size_t at = 0; at < num_g2; at += slice) {
                const size_t cnt = num_g2 - at < slice ? num_g2 - at : slice;
                enqueue_powers((Fr*)w.sc.p, s, one, at, cnt, st.st);
                enqueue_g2_mul(w.pts.p, (const Fr*)w.sc.p, tab, cnt, st.st);
                DEV_TRY(hipGetLastError());
                DEV_TRY(hipMemcpyAsync(g2_monomial + at, w.pts.p, cnt * sizeof(blst_p2), hipMemcpyDeviceToHost, st.st));
                DEV_TRY(hipStreamSynchronize(st.st));
            }
        }
    });
}
