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
#include "host_call.h"
#include "host_fp64.h"
#include "host_g1.h"
#include "msm_internal.h"
#include "ntt_internal.h"

using ff::Fr;
using ff::u32;
using g1::Xyzz;
using kzgamd::blocks;
using kzgamd::DevBuf;
using kzgamd::DevErr;
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
    DevBuf x;                             // direct form: X[j][i], k2 * l points
    kzgamd::MsmContext* msm = nullptr;    // table form: the same points as k2 base sets of l
    // workspace of a pass of `cap` polynomials
    size_t cap = 0;
    DevBuf poly, t, f, sc, prod, tab, h, h2, out;

    void drop_workspace() {
        kzgamd::drop_all(poly, t, f, sc, prod, tab, h, h2, out);
        cap = 0;
    }
    void ensure(size_t npoly) {
        if (npoly <= cap) return;
        drop_workspace();
        const size_t nprod = npoly * 2 * n, npos = npoly * k2;
        poly.ensure(npoly * n * sizeof(Fr));
        t.ensure(nprod * sizeof(Fr));
        f.ensure(nprod * sizeof(Fr));
        sc.ensure(nprod * sizeof(RootSplit));
        if (form == 1 && l > 1) prod.ensure(nprod * sizeof(Xyzz));
        // lane tables: 9 slots per half-product (direct form) or per half-butterfly of the G1 transforms
        tab.ensure(9 * (form == 1 ? 2 * nprod : npos) * sizeof(Xyzz));
        h.ensure(npos * sizeof(Xyzz));
        h2.ensure(npos * sizeof(Xyzz));
        out.ensure(npos * sizeof(blst_p1));
        cap = npoly;
    }
    ~Fk20Ctx() {
        if (msm) kzgamd::msm_destroy(msm);
        if (st) (void)hipStreamDestroy(st);
    }
};

// X[j][i] on the device from the monomial setup points: one batched G1 transform of l x k2 points
void build_x(Fk20Ctx* fk, const blst_p1* mono) {
    const size_t n = fk->n, l = fk->l, k = fk->k, k2 = fk->k2, total = l * k2;
    std::vector<blst_p1> x(total);
    memset(x.data(), 0, total * sizeof(blst_p1));  // Z == 0: the identity
    for (size_t i = 0; i < l; ++i)
        for (size_t m = 0; m + 1 < k; ++m) x[i * k2 + m] = mono[n - l - 1 - i - l * m];
    kzgamd::ScopedBuf p1, a, b, tab;
    try {
        p1.alloc(total * sizeof(blst_p1));
        a.alloc(total * sizeof(Xyzz));
        b.alloc(total * sizeof(Xyzz));
        tab.alloc(9 * total * sizeof(Xyzz));
        fk->x.ensure(total * sizeof(Xyzz));
        DEV_TRY(hipMemcpyAsync(p1.p, x.data(), total * sizeof(blst_p1), hipMemcpyHostToDevice, fk->st));
        kzgamd::g1_jacobian_to_xyzz(a.p, p1.p, total, fk->st);
        void* res = kzgamd::fftg1_device_tab(fk->ntt, a.p, b.p, k2, l, 0, fk->st, tab.p);
        if (!res) throw DevErr{hipErrorOutOfMemory};
        hipLaunchKernelGGL(k_fk20g_transpose_x, dim3(blocks(total)), dim3(256), 0, fk->st, fk->x.as<Xyzz>(), (const Xyzz*)res, l, k2);
        DEV_TRY(hipGetLastError());
        DEV_TRY(hipStreamSynchronize(fk->st));
    } catch (...) {
        (void)hipStreamSynchronize(fk->st);  // before the buffers of the call go
        throw;
    }
}

// the table form: X[j][i] as affine points on the host -> a wide fixed-base table of k2 base sets of l points.
// false: no table fits.
bool build_table(Fk20Ctx* fk, const kzgamd::Options& opt) {
    const size_t total = fk->k2 * fk->l;
    if (!kzgamd::msm_wide_table_fits(total, &opt)) return false;
    std::vector<blst_p1> jac(total);
    std::vector<ff::Fp> aff(2 * total);
    {
        kzgamd::ScopedBuf p1;
        p1.alloc(total * sizeof(blst_p1));
        kzgamd::g1_xyzz_to_jacobian(p1.p, fk->x.p, total, fk->st);
        DEV_TRY(hipMemcpyAsync(jac.data(), p1.p, total * sizeof(blst_p1), hipMemcpyDeviceToHost, fk->st));
        DEV_TRY(hipStreamSynchronize(fk->st));
    }
    kzgamd::host_p1_to_affine_batch(aff.data(), total, [&](size_t i) { return &jac[i]; });
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
    Fr *d_t = fk->t.as<Fr>(), *d_f = fk->f.as<Fr>();
    Xyzz *d_h = fk->h.as<Xyzz>(), *d_h2 = fk->h2.as<Xyzz>(), *d_tab = fk->tab.as<Xyzz>();
    DEV_TRY(hipMemcpyAsync(fk->poly.p, polys, cnt * n * sizeof(Fr), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_fk20g_toeplitz, dim3(blocks(nprod)), dim3(256), 0, st, d_t, (const Fr*)fk->poly.p, n, l, k, nprod);
    if (kzgamd_ntt_fr_device(fk->ntt, d_f, d_t, k2, l * cnt, 0, st) != 0) throw DevErr{hipErrorUnknown};
    hipLaunchKernelGGL(k_fk20g_scalars, dim3(blocks(nprod)), dim3(256), 0, st, fk->sc.p, (const Fr*)d_f, l, k2, fk->inv_k2,
                       fk->form == 1 ? 1 : 0, nprod);
    if (fk->form == 1) {
        kzgamd::g1_varmul_sum_device(fk->ntt, d_h, fk->prod.p, d_tab, fk->x.p, k2 * l, (const RootSplit*)fk->sc.p, nprod, l, st);
    } else {
        // h_ext[poly][j] = sum_i scalars[poly][j][i] * X[j][i]: cnt * k2 MSMs of l points, base set j of the table
        kzgamd::MsmLock locked(fk->msm);
        kzgamd::msm_enqueue(fk->msm, d_h, fk->sc.p, l, npos, 1, st, kzgamd::OUT_XYZZ, false, k2);
    }
    // h = ifft_g1(h_ext) (its k2^-1 is in the scalars), upper half cleared, proofs = fft_g1(h)
    Xyzz* h = (Xyzz*)kzgamd::fftg1_device_tab(fk->ntt, d_h, d_h2, k2, cnt, 1, st, d_tab);
    if (!h) throw DevErr{hipErrorUnknown};
    Xyzz* other = h == d_h ? d_h2 : d_h;
    hipLaunchKernelGGL(k_fk20g_zero_upper, dim3(blocks(cnt * k)), dim3(256), 0, st, h, k, cnt * k);
    Xyzz* pr = (Xyzz*)kzgamd::fftg1_device_tab(fk->ntt, h, other, k2, cnt, 0, st, d_tab);
    if (!pr) throw DevErr{hipErrorUnknown};
    if (!optimized) {
        Xyzz* fin = pr == h ? other : h;
        hipLaunchKernelGGL(k_fk20g_brp, dim3(blocks(npos)), dim3(256), 0, st, fin, (const Xyzz*)pr, k2, fk->logk2, npos);
        pr = fin;
    }
    kzgamd::g1_xyzz_to_jacobian(fk->out.p, pr, npos, st);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipMemcpyAsync(out, fk->out.p, npos * sizeof(blst_p1), hipMemcpyDeviceToHost, st));
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
    long long want = -1;
    KzgAmdConfig local;
    std::string rest, msg;
    if (cfg && cfg->struct_size >= offsetof(KzgAmdConfig, tuning) + sizeof(cfg->tuning) && cfg->tuning) {
        if (!kzgamd::take_key(cfg->tuning, "fk20_table", -1, 1, &want, &rest)) {
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
    Fk20Ctx* fk = kzgamd::create_handle<Fk20Ctx>(ntt->device, err, [&](Fk20Ctx* fk) {
        fk->ntt = ntt;
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
        DEV_TRY(hipStreamCreateWithFlags(&fk->st, hipStreamNonBlocking));
        build_x(fk, g1_monomial);
        if (want != 0 && build_table(fk, opt)) {
            fk->form = 2;
            fk->x.drop();  // the table holds the points now
        }
    });
    if (fk && want == 1 && fk->form != 2) {
        fprintf(stderr, "kzg_mi355x: kzgamd_fk20_new: fk20_table=1, but no wide table of %zu x %zu points fits the budget\n", fk->k2,
                fk->l);
        *err = -3;
        kzgamd_fk20_free(fk);
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
    return kzgamd::run_call(fk, [&] {
        size_t per = CHUNK_PRODUCTS / (2 * fk->n);
        if (per == 0) per = 1;
        if (per > npoly) per = npoly;
        fk->ensure(per);
        for (size_t done = 0; done < npoly; done += per) {
            const size_t cnt = npoly - done < per ? npoly - done : per;
            run_pass(fk, out + done * fk->k2, polys + done * fk->n, cnt, optimized);
        }
    });
}
