// Generic FK20 data-availability proofs: FK20SingleSettings / FK20MultiSettings of the reference
// (blst/src/types/fk20_single_settings.rs:38-111, blst/src/types/fk20_multi_settings.rs:60-175, blst/src/fk20_proofs.rs:16-93)
// for any polynomial length n = n2 / 2 and chunk length l (the single form is l = 1), npoly polynomials per call.
//
// With k = n / l, k2 = 2k:
//   setup, once:  x_i = (mono[n-l-1-i], mono[n-2l-1-i], ..., k - 1 of them, identity), zero-extended to k2, X_i = fft_g1(x_i)
//                 for every offset i < l — ONE batched G1 transform of l x k2 points, kept on the device as X[j][i];
//   per call:     t_i = toeplitz_coeffs_stride(p, i, l) -> fft (Fr, l * npoly transforms of k2) ->
//                 h_ext[j] = sum_i fft(t_i)[j] * X_i[j] -> inverse fft_g1, upper half := identity -> fft_g1 -> (bit reversal).
// The reference spends the call in the 2n scalar multiplications of the pointwise products and the two G1 transforms.
// The products come in two forms:
//   direct (1): a scalar multiplication per product whose scalar is read from device memory (k_g1_varmul_* of fftg1.hip:
//               the transformed coefficients, split into their GLV halves on the device by k_fk20g_scalars), then a
//               tree sum over the l products of a position;
//   table  (2): the k2 x l points as a matrix of k2 base sets in a wide fixed-base table (the form of the EIP-7594 cell
//               proofs, ckzg_7594.hip), when that table fits the handle's budget.
// Everything between the upload of the coefficients and the download of the proofs is enqueued on the handle's one
// stream; a call holds the handle's lock and synchronises before it returns.  The G1 transforms run with per-lane tables
// of this handle (fftg1_device_tab), so fft_g1 calls on the NTT handle underneath run beside it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/kzg_mi355x.h"
#include "config.h"
#include "device_guard.h"
#include "ff.hip.h"
#include "g1_28.hip.h"
#include "glv.hip.h"
#include "host_fp64.h"
#include "msm_internal.h"
#include "ntt_internal.h"

using ff::Fr;
using ff::u32;
using g1::Xyzz;
using kzgamd::RootSplit;

namespace {

// toeplitz_coeffs_stride(p, i, l) for every (polynomial, offset i < l): a k2-vector with p[n - 1 - i] at 0 and
// p[n - 1 - i - l (k2 - idx)] at idx = k + 2 .. k2 - 1 (fk20_proofs.rs:65-88; nothing but the head for k <= 2)
__global__ void __launch_bounds__(256) k_fk20g_toeplitz(Fr* __restrict__ out, const Fr* __restrict__ polys, size_t n, size_t l,
                                                        size_t k, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // total = npoly * l * k2
    if (t >= total) return;
    const size_t k2 = 2 * k;
    const size_t idx = t % k2, i = (t / k2) % l, b = t / (k2 * l);
    const Fr* p = polys + b * n;
    Fr v = Fr::zero();
    if (idx == 0) v = p[n - 1 - i];
    else if (idx >= k + 2) v = p[n - 1 - i - l * (k2 - idx)];
    out[t] = v;
}

// the scalars of the pointwise products next to each other per position: (poly, j, i) <- transform_i[j] / k2 (the k2^-1
// of the inverse G1 transform that follows folded in).  split: as 48-byte RootSplit records, the GLV halves the
// multiplication kernels read; else as Montgomery Fr for the fixed-base engine.
__global__ void __launch_bounds__(256) k_fk20g_scalars(void* __restrict__ out, const Fr* __restrict__ in, size_t l, size_t k2,
                                                       Fr inv_k2, int split, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // total = npoly * k2 * l
    if (t >= total) return;
    const size_t i = t % l, j = (t / l) % k2, b = t / (l * k2);
    const Fr v = ff::mul(in[(b * l + i) * k2 + j], inv_k2);
    if (!split) {
        ((Fr*)out)[t] = v;
        return;
    }
    const Fr plain = ff::from_mont(v);
    u32 k1[8], k2h[8], n1, n2;
    kzgamd::glv_split(plain.v, k1, k2h, n1, n2);
    RootSplit rs;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        rs.k[0][w] = k1[w];
        rs.k[1][w] = k2h[w];
    }
    rs.neg[0] = n1;
    rs.neg[1] = n2;
    rs.pad[0] = rs.pad[1] = 0;
    ((RootSplit*)out)[t] = rs;
}

// X_i[j] (transform-major, as the batched transform leaves it) -> X[j][i], the order of the products of a position
__global__ void __launch_bounds__(256) k_fk20g_transpose_x(Xyzz* __restrict__ out, const Xyzz* __restrict__ in, size_t l, size_t k2) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= l * k2) return;
    const size_t i = t % l, j = t / l;
    out[t] = in[i * k2 + j];
}
// h[k .. k2) = identity for every polynomial
__global__ void __launch_bounds__(256) k_fk20g_zero_upper(Xyzz* __restrict__ h, size_t k, size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // total = npoly * k
    if (t >= total) return;
    g1::set_inf(h[(t / k) * 2 * k + k + t % k]);
}
// reverse_bit_order of the k2 proofs of every polynomial
__global__ void __launch_bounds__(256) k_fk20g_brp(Xyzz* __restrict__ out, const Xyzz* __restrict__ in, size_t k2, int logk2,
                                                   size_t total) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const u32 j = (u32)(t % k2);
    const u32 r = logk2 == 0 ? 0u : __builtin_bitreverse32(j) >> (32 - logk2);
    out[t] = in[t - j + r];
}

struct FkErr {
    hipError_t e;
};
#define FK_TRY(x)                              \
    do {                                       \
        hipError_t _e = (x);                   \
        if (_e != hipSuccess) throw FkErr{_e}; \
    } while (0)

constexpr size_t CHUNK_PRODUCTS = (size_t)1 << 19;  // products per pass of a call: bounds the workspace (2.2 GB of lane tables)

struct Fk20Ctx {
    NttCtx* ntt = nullptr;
    int device = 0;
    size_t n2 = 0, n = 0, l = 0, k = 0, k2 = 0;
    int logk2 = 0;
    int form = 1;
    Fr inv_k2;
    std::mutex mu;
    hipStream_t st = nullptr;
    Xyzz* d_x = nullptr;                  // direct form: X[j][i], k2 * l points
    kzgamd::MsmContext* msm = nullptr;    // table form: the same points as k2 base sets of l
    // workspace of a pass of `cap` polynomials
    size_t cap = 0;
    Fr *d_poly = nullptr, *d_t = nullptr, *d_f = nullptr;
    void* d_sc = nullptr;
    Xyzz *d_prod = nullptr, *d_tab = nullptr, *d_h = nullptr, *d_h2 = nullptr;
    void* d_out = nullptr;

    void drop_workspace() {
        void* all[] = {d_poly, d_t, d_f, d_sc, d_prod, d_tab, d_h, d_h2, d_out};
        for (void* p : all)
            if (p) (void)hipFree(p);
        d_poly = d_t = d_f = nullptr;
        d_sc = d_out = nullptr;
        d_prod = d_tab = d_h = d_h2 = nullptr;
        cap = 0;
    }
    void ensure(size_t npoly) {
        if (npoly <= cap) return;
        drop_workspace();
        const size_t nprod = npoly * 2 * n, npos = npoly * k2;
        FK_TRY(hipMalloc(&d_poly, npoly * n * sizeof(Fr)));
        FK_TRY(hipMalloc(&d_t, nprod * sizeof(Fr)));
        FK_TRY(hipMalloc(&d_f, nprod * sizeof(Fr)));
        FK_TRY(hipMalloc(&d_sc, nprod * sizeof(RootSplit)));
        if (form == 1 && l > 1) FK_TRY(hipMalloc(&d_prod, nprod * sizeof(Xyzz)));
        // lane tables: 9 slots per half-product (direct form) or per half-butterfly of the G1 transforms
        FK_TRY(hipMalloc(&d_tab, 9 * (form == 1 ? 2 * nprod : npos) * sizeof(Xyzz)));
        FK_TRY(hipMalloc(&d_h, npos * sizeof(Xyzz)));
        FK_TRY(hipMalloc(&d_h2, npos * sizeof(Xyzz)));
        FK_TRY(hipMalloc(&d_out, npos * sizeof(blst_p1)));
        cap = npoly;
    }
    ~Fk20Ctx() {
        drop_workspace();
        if (d_x) (void)hipFree(d_x);
        if (msm) kzgamd::msm_destroy(msm);
        if (st) (void)hipStreamDestroy(st);
    }
};

inline unsigned blocks(size_t total) { return (unsigned)((total + 255) / 256); }

// "fk20_table=<v>" out of a "key=value;key=value" tuning string (separators as config.h takes them): *value is set when
// the key is there, *rest is the string without it; false when its value is not -1, 0 or 1
bool take_fk20_table(const char* str, long* value, std::string* rest) {
    static const char key[] = "fk20_table";
    auto is_sep = [](char c) { return c == ';' || c == ',' || c == ' ' || c == '\t' || c == '\n'; };
    const char* p = str;
    while (*p) {
        while (*p && is_sep(*p)) ++p;
        const char* e = p;
        while (*e && !is_sep(*e)) ++e;
        if (e == p) break;
        if ((size_t)(e - p) > sizeof key - 1 && !strncmp(p, key, sizeof key - 1) && p[sizeof key - 1] == '=') {
            char* end = nullptr;
            const long v = strtol(p + sizeof key, &end, 10);
            if (end != e || end == p + sizeof key || v < -1 || v > 1) return false;
            *value = v;
        } else {
            if (!rest->empty()) *rest += ';';
            rest->append(p, e);
        }
        p = e;
    }
    return true;
}

// X[j][i] on the device from the monomial setup points: one batched G1 transform of l x k2 points
void build_x(Fk20Ctx* fk, const blst_p1* mono) {
    const size_t n = fk->n, l = fk->l, k = fk->k, k2 = fk->k2, total = l * k2;
    std::vector<blst_p1> x(total);
    memset(x.data(), 0, total * sizeof(blst_p1));  // Z == 0: the identity
    for (size_t i = 0; i < l; ++i)
        for (size_t m = 0; m + 1 < k; ++m) x[i * k2 + m] = mono[n - l - 1 - i - l * m];
    void *d_p1 = nullptr, *d_a = nullptr, *d_b = nullptr, *d_tab = nullptr;
    try {
        FK_TRY(hipMalloc(&d_p1, total * sizeof(blst_p1)));
        FK_TRY(hipMalloc(&d_a, total * sizeof(Xyzz)));
        FK_TRY(hipMalloc(&d_b, total * sizeof(Xyzz)));
        FK_TRY(hipMalloc(&d_tab, 9 * total * sizeof(Xyzz)));
        FK_TRY(hipMalloc(&fk->d_x, total * sizeof(Xyzz)));
        FK_TRY(hipMemcpyAsync(d_p1, x.data(), total * sizeof(blst_p1), hipMemcpyHostToDevice, fk->st));
        kzgamd::g1_jacobian_to_xyzz(d_a, d_p1, total, fk->st);
        void* res = kzgamd::fftg1_device_tab(fk->ntt, d_a, d_b, k2, l, 0, fk->st, d_tab);
        if (!res) throw FkErr{hipErrorOutOfMemory};
        hipLaunchKernelGGL(k_fk20g_transpose_x, dim3(blocks(total)), dim3(256), 0, fk->st, fk->d_x, (const Xyzz*)res, l, k2);
        FK_TRY(hipGetLastError());
        FK_TRY(hipStreamSynchronize(fk->st));
    } catch (...) {
        (void)hipStreamSynchronize(fk->st);
        for (void* p : {d_p1, d_a, d_b, d_tab})
            if (p) (void)hipFree(p);
        throw;
    }
    for (void* p : {d_p1, d_a, d_b, d_tab}) (void)hipFree(p);
}

// the table form: X[j][i] as affine points on the host (Montgomery's trick over the Z coordinates; the identity as
// (0, 0), blst's affine infinity) -> a wide fixed-base table of k2 base sets of l points.  false: no table fits.
bool build_table(Fk20Ctx* fk, const kzgamd::Options& opt) {
    const size_t total = fk->k2 * fk->l;
    if (!kzgamd::msm_wide_table_fits(total, &opt)) return false;
    std::vector<ff::Fp> jac(3 * total), aff(2 * total), pre(total);
    void* d_p1 = nullptr;
    FK_TRY(hipMalloc(&d_p1, total * sizeof(blst_p1)));
    kzgamd::g1_xyzz_to_jacobian(d_p1, fk->d_x, total, fk->st);
    hipError_t e = hipMemcpyAsync(jac.data(), d_p1, total * sizeof(blst_p1), hipMemcpyDeviceToHost, fk->st);
    if (e == hipSuccess) e = hipStreamSynchronize(fk->st);
    (void)hipFree(d_p1);
    FK_TRY(e);
    ff::Fp run = ff::Fp::one();
    for (size_t i = 0; i < total; ++i) {
        pre[i] = run;
        if (!jac[3 * i + 2].is_zero()) run = hfp::mul(run, jac[3 * i + 2]);
    }
    ff::Fp inv = ff::inverse_bgcd(run);
    for (size_t i = total; i-- > 0;) {
        const ff::Fp* P = &jac[3 * i];
        if (P[2].is_zero()) {
            aff[2 * i] = aff[2 * i + 1] = ff::Fp::zero();
            continue;
        }
        const ff::Fp zi = hfp::mul(inv, pre[i]), zi2 = hfp::sqr(zi);
        inv = hfp::mul(inv, P[2]);
        aff[2 * i] = hfp::mul(P[0], zi2);
        aff[2 * i + 1] = hfp::mul(P[1], hfp::mul(zi2, zi));
    }
    kzgamd::MsmContext* m = nullptr;
    try {
        m = kzgamd::msm_create(aff.data(), total, false, true, false, kzgamd::G1_TRUSTED, &opt);
    } catch (...) {
        return false;
    }
    if (!kzgamd::msm_has_wide_table(m)) {
        kzgamd::msm_destroy(m);
        return false;
    }
    fk->msm = m;
    return true;
}

// one pass: `cnt` polynomials, host to host
void run_pass(Fk20Ctx* fk, blst_p1* out, const blst_fr* polys, size_t cnt, int optimized) {
    const size_t n = fk->n, l = fk->l, k = fk->k, k2 = fk->k2;
    const size_t nprod = cnt * k2 * l, npos = cnt * k2;
    hipStream_t st = fk->st;
    FK_TRY(hipMemcpyAsync(fk->d_poly, polys, cnt * n * sizeof(Fr), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_fk20g_toeplitz, dim3(blocks(nprod)), dim3(256), 0, st, fk->d_t, (const Fr*)fk->d_poly, n, l, k, nprod);
    if (kzgamd_ntt_fr_device(fk->ntt, fk->d_f, fk->d_t, k2, l * cnt, 0, st) != 0) throw FkErr{hipErrorUnknown};
    hipLaunchKernelGGL(k_fk20g_scalars, dim3(blocks(nprod)), dim3(256), 0, st, fk->d_sc, (const Fr*)fk->d_f, l, k2, fk->inv_k2,
                       fk->form == 1 ? 1 : 0, nprod);
    if (fk->form == 1) {
        kzgamd::g1_varmul_sum_device(fk->ntt, fk->d_h, fk->d_prod, fk->d_tab, fk->d_x, k2 * l, (const RootSplit*)fk->d_sc, nprod, l, st);
    } else {
        // h_ext[poly][j] = sum_i scalars[poly][j][i] * X[j][i]: cnt * k2 MSMs of l points, base set j of the table
        kzgamd::msm_lock(fk->msm);
        try {
            kzgamd::msm_enqueue(fk->msm, fk->d_h, fk->d_sc, l, npos, 1, st, kzgamd::OUT_XYZZ, false, k2);
        } catch (...) {
            kzgamd::msm_unlock(fk->msm);
            throw FkErr{hipErrorUnknown};
        }
        kzgamd::msm_unlock(fk->msm);
    }
    // h = ifft_g1(h_ext) (its k2^-1 is in the scalars), upper half cleared, proofs = fft_g1(h)
    Xyzz* h = (Xyzz*)kzgamd::fftg1_device_tab(fk->ntt, fk->d_h, fk->d_h2, k2, cnt, 1, st, fk->d_tab);
    if (!h) throw FkErr{hipErrorUnknown};
    Xyzz* other = h == fk->d_h ? fk->d_h2 : fk->d_h;
    hipLaunchKernelGGL(k_fk20g_zero_upper, dim3(blocks(cnt * k)), dim3(256), 0, st, h, k, cnt * k);
    Xyzz* pr = (Xyzz*)kzgamd::fftg1_device_tab(fk->ntt, h, other, k2, cnt, 0, st, fk->d_tab);
    if (!pr) throw FkErr{hipErrorUnknown};
    if (!optimized) {
        Xyzz* fin = pr == h ? other : h;
        hipLaunchKernelGGL(k_fk20g_brp, dim3(blocks(npos)), dim3(256), 0, st, fin, (const Xyzz*)pr, k2, fk->logk2, npos);
        pr = fin;
    }
    kzgamd::g1_xyzz_to_jacobian(fk->d_out, pr, npos, st);
    FK_TRY(hipGetLastError());
    FK_TRY(hipMemcpyAsync(out, fk->d_out, npos * sizeof(blst_p1), hipMemcpyDeviceToHost, st));
}

}  // namespace

extern "C" void* kzgamd_fk20_new(void* vntt, const blst_p1* g1_monomial, size_t num_g1, size_t n2, size_t chunk_len,
                                 const KzgAmdConfig* cfg, int* err) {
    int dummy;
    if (!err) err = &dummy;
    *err = 0;
    NttCtx* ntt = (NttCtx*)vntt;
    if (!ntt || !g1_monomial) {
        *err = -1;
        return nullptr;
    }
    // the reference's checks in the reference's order (fk20_multi_settings.rs:61-73)
    if (n2 > ntt->W) *err = 1;
    else if (n2 == 0 || (n2 & (n2 - 1))) *err = 2;
    else if (n2 < 2) *err = 3;
    else if (chunk_len > n2 / 2) *err = 4;
    else if (chunk_len == 0 || (chunk_len & (chunk_len - 1))) *err = 5;
    else if (num_g1 < n2 / 2 - chunk_len) *err = 6;
    if (*err) return nullptr;
    // fk20_table is a key of this handle type alone: it is taken out of cfg->tuning here, the rest goes to the library's
    // table of keys (config.h) as for every other handle
    long want = -1;
    KzgAmdConfig local;
    std::string rest, msg;
    if (cfg && cfg->struct_size >= offsetof(KzgAmdConfig, tuning) + sizeof(cfg->tuning) && cfg->tuning) {
        if (!take_fk20_table(cfg->tuning, &want, &rest)) {
            fprintf(stderr, "kzg_mi355x: kzgamd_fk20_new: tuning: 'fk20_table' takes -1, 0 or 1\n");
            *err = -2;
            return nullptr;
        }
        local = *cfg;
        local.tuning = rest.c_str();
        cfg = &local;
    }
    kzgamd::Options opt;
    if (!kzgamd::Options::resolve(opt, cfg, &msg)) {
        fprintf(stderr, "kzg_mi355x: kzgamd_fk20_new: %s\n", msg.c_str());
        *err = -2;
        return nullptr;
    }
    opt.device = ntt->device;  // the handle lives where its NTT handle lives
    auto* fk = new Fk20Ctx();
    try {
        kzgamd::DeviceGuard on_device(ntt->device);
        FK_TRY(on_device.err);
        fk->ntt = ntt;
        fk->device = ntt->device;
        fk->n2 = n2;
        fk->n = n2 / 2;
        fk->l = chunk_len;
        fk->k = fk->n / chunk_len;
        fk->k2 = 2 * fk->k;
        while (((size_t)1 << fk->logk2) < fk->k2) ++fk->logk2;
        Fr v = Fr::zero();
        v.v[0] = (u32)fk->k2;
        v.v[1] = (u32)((uint64_t)fk->k2 >> 32);
        fk->inv_k2 = ff::inverse_bgcd(ff::to_mont(v));  // Montgomery form of 1 / k2
        FK_TRY(hipStreamCreateWithFlags(&fk->st, hipStreamNonBlocking));
        build_x(fk, g1_monomial);
        if (want != 0 && build_table(fk, opt)) {
            fk->form = 2;
            (void)hipFree(fk->d_x);  // the table holds the points now
            fk->d_x = nullptr;
        } else if (want == 1) {
            fprintf(stderr, "kzg_mi355x: kzgamd_fk20_new: fk20_table=1, but no wide table of %zu x %zu points fits the budget\n",
                    fk->k2, fk->l);
            *err = -3;
            delete fk;
            return nullptr;
        }
    } catch (const FkErr& e) {
        *err = -(int)e.e - 100;
        kzgamd::DeviceGuard on_device(ntt->device);
        delete fk;
        return nullptr;
    } catch (...) {
        *err = -4;
        kzgamd::DeviceGuard on_device(ntt->device);
        delete fk;
        return nullptr;
    }
    return fk;
}

extern "C" void kzgamd_fk20_free(void* vfk) {
    Fk20Ctx* fk = (Fk20Ctx*)vfk;
    if (!fk) return;
    kzgamd::DeviceGuard on_device(fk->device);
    delete fk;
}

extern "C" int kzgamd_fk20_info(void* vfk, size_t* n2, size_t* chunk_len, int* form) {
    Fk20Ctx* fk = (Fk20Ctx*)vfk;
    if (!fk) return -1;
    if (n2) *n2 = fk->n2;
    if (chunk_len) *chunk_len = fk->l;
    if (form) *form = fk->form;
    return 0;
}

extern "C" int kzgamd_fk20_da(void* vfk, blst_p1* out, const blst_fr* polys, size_t n, size_t npoly, int optimized) {
    Fk20Ctx* fk = (Fk20Ctx*)vfk;
    if (!fk) return -1;
    if (n != fk->n) return 3;
    if (npoly == 0) return 0;
    if (!out || !polys) return -1;
    std::lock_guard<std::mutex> lk(fk->mu);
    int rc = 0;
    try {
        kzgamd::DeviceGuard on_device(fk->device);
        FK_TRY(on_device.err);
        size_t per = CHUNK_PRODUCTS / (2 * fk->n);
        if (per == 0) per = 1;
        if (per > npoly) per = npoly;
        fk->ensure(per);
        try {
            for (size_t done = 0; done < npoly; done += per) {
                const size_t cnt = npoly - done < per ? npoly - done : per;
                run_pass(fk, out + done * fk->k2, polys + done * fk->n, cnt, optimized);
            }
        } catch (...) {
            (void)hipStreamSynchronize(fk->st);  // a copy into the caller's buffer may be in flight
            throw;
        }
        FK_TRY(hipStreamSynchronize(fk->st));
    } catch (const FkErr& e) {
        rc = -(int)e.e - 100;
    } catch (...) {
        rc = -2;
    }
    return rc;
}
