// Batched pairing checks on the GPU: e(a1[i], A2) == e(b1[i], B2) for many i against two shared G2 points, ONE WAVE PER
// CHECK.  A check is a single chain of ~5 000 dependent multiplication steps (Miller loop over two cached line tables,
// final exponentiation), so a wave runs it with the limbs of Fp across the lanes of a DPP row and four independent Fp
// products per step (fp12w.hip.h); the batch supplies the parallelism across waves.  host_pairing.h is the
// specification: verdicts equal pairing::pairings_verify's for every input.
#include <hip/hip_runtime.h>
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "device_guard.h"
#include "fp12w.hip.h"
#include "host_call.h"
#include "host_pairing.h"
#include "pairing_internal.h"

namespace {
using ff::u32;
namespace hp = kzgamd::pairing;
using kzgamd::pairing_gpu::DeviceTable;
using kzgamd::pairing_gpu::SLICE;

// One wave per block, so every LDS word of the block belongs to the wave and no workgroup barrier is needed anywhere.
__global__ void __launch_bounds__(64) k_pairing_check(uint8_t* __restrict__ ok, const blst_p1* __restrict__ a1,
                                                      const blst_p1* __restrict__ b1, const u32* __restrict__ tab_a,
                                                      const u32* __restrict__ tab_b, const u32* __restrict__ prog, int nprog,
                                                      const u32* __restrict__ frob, unsigned count) {
    __shared__ u32 sh[fp12w::WAVE_WORDS];
    const unsigned i = blockIdx.x;
    if (i >= count) return;
    const int lane = threadIdx.x;
    const fp12w::Ctx c = fp12w::make_ctx(lane);
    fp12w::Pairs pr;
    pr.tab[0] = tab_a;
    pr.tab[1] = tab_b;
    fp12w::pairs_prepare(pr, sh, (const u32*)(a1 + i), (const u32*)(b1 + i), c);
    if (pr.skip[0] && pr.skip[1]) {  // the empty product
        if (lane == 0) ok[i] = 1;
        return;
    }
    fp12w::run_program(prog, nprog, sh, pr, frob, c);
    const bool one = fp12w::f12_is_one(fp12w::f12_load(sh, 0, c), c, fp12w::xchg_words(sh));
    if (lane == 0) ok[i] = one ? 1 : 0;
}

// ---- host side: the program, the constants, the tables
void put_fp(u32* dst16, const ff::Fp& a) {
    const fp28::Fe f = fp28::canon(fp28::from_blst(a));
    for (int k = 0; k < fp28::L; ++k) dst16[k] = f.v[k];
    dst16[14] = dst16[15] = 0;
}

// slots: 0 = f (the Miller value, then the result), 1..7 = t0..t6 of final_exponentiation, 8 and 9 = temporaries
std::vector<u32> build_program() {
    using namespace fp12w;
    std::vector<u32> p;
    enum { F = 0, T0, T1, T2, T3, T4, T5, T6, A, B };
    // miller_loop_multi: one squaring per bit, one line per pair and step (both pairs inside OP_LINE), conjugated
    p.push_back(insn(OP_ONE, F, 0));
    u32 idx = 0;
    for (int bit = 62; bit >= 0; --bit) {
        p.push_back(insn(OP_SQR, F, F));
        p.push_back(insn(OP_LINE, F, F, idx++));
        if ((hp::BLS_X_ABS >> bit) & 1) p.push_back(insn(OP_LINE, F, F, idx++));
    }
    p.push_back(insn(OP_CONJ, F, F));
    auto exp_x = [&](u32 d, u32 a) {  // d != a
        for (int bit = 62; bit >= 0; --bit) {
            p.push_back(insn(OP_CSQR, d, bit == 62 ? a : d));
            if ((hp::BLS_X_ABS >> bit) & 1) p.push_back(insn(OP_MUL, d, d, a));
        }
        p.push_back(insn(OP_CONJ, d, d));
    };
    // final_exponentiation, line by line
    p.push_back(insn(OP_CONJ, A, F));
    p.push_back(insn(OP_INV, B, F));
    p.push_back(insn(OP_MUL, T2, A, B));
    p.push_back(insn(OP_FROB, A, T2));
    p.push_back(insn(OP_FROB, A, A));
    p.push_back(insn(OP_MUL, T2, A, T2));
    p.push_back(insn(OP_CSQR, T1, T2));
    p.push_back(insn(OP_CONJ, T1, T1));
    exp_x(T3, T2);
    p.push_back(insn(OP_CSQR, T4, T3));
    p.push_back(insn(OP_MUL, T5, T1, T3));
    exp_x(T1, T5);
    exp_x(T0, T1);
    exp_x(A, T0);
    p.push_back(insn(OP_MUL, T6, A, T4));
    exp_x(T4, T6);
    p.push_back(insn(OP_CONJ, T5, T5));
    p.push_back(insn(OP_MUL, A, T5, T2));
    p.push_back(insn(OP_MUL, T4, T4, A));
    p.push_back(insn(OP_CONJ, T5, T2));
    p.push_back(insn(OP_MUL, T1, T1, T2));
    p.push_back(insn(OP_FROB, T1, T1));
    p.push_back(insn(OP_FROB, T1, T1));
    p.push_back(insn(OP_FROB, T1, T1));
    p.push_back(insn(OP_MUL, A, T6, T5));
    p.push_back(insn(OP_FROB, T6, A));
    p.push_back(insn(OP_MUL, A, T3, T0));
    p.push_back(insn(OP_FROB, A, A));
    p.push_back(insn(OP_FROB, T3, A));
    p.push_back(insn(OP_MUL, A, T3, T1));
    p.push_back(insn(OP_MUL, A, A, T6));
    p.push_back(insn(OP_MUL, F, A, T4));
    p.push_back(insn(OP_END, 0, 0));
    return p;
}

struct HipFree {
    void operator()(void* p) const { (void)hipFree(p); }
};

// Workspaces, the per-device program and constants live as long as the process (a few hundred KB per device and per call
// that was ever in flight at once); line tables are freed when they leave the cache and their last user is done.
struct Workspace {  // what one call in flight owns
    hipStream_t st = nullptr;
    blst_p1* pts = nullptr;  // 2 * SLICE
    uint8_t* ok = nullptr;   // SLICE
};
struct PerDevice {
    u32* prog = nullptr;
    int nprog = 0;
    u32* frob = nullptr;
    std::vector<Workspace> idle;
};
struct TableEntry {
    int device;
    hp::G2Jac key;
    std::shared_ptr<void> words;  // nullptr for infinity
};
std::mutex g_mu;
std::map<int, PerDevice> g_dev;
std::vector<TableEntry> g_tables;

hipError_t per_device(PerDevice** out, int device) {  // g_mu held
    auto it = g_dev.find(device);
    if (it != g_dev.end()) {
        *out = &it->second;
        return hipSuccess;
    }
    const std::vector<u32> prog = build_program();
    std::vector<u32> frob(fp12w::FROB_WORDS);
    const hp::FrobeniusConstants& k = hp::frobenius_constants();
    for (int i = 0; i < 6; ++i) {
        put_fp(&frob[(2 * i) * 16], k.g[i].c0);
        put_fp(&frob[(2 * i + 1) * 16], k.g[i].c1);
    }
    PerDevice d;
    hipError_t e = hipMalloc((void**)&d.prog, prog.size() * sizeof(u32));
    if (e == hipSuccess) e = hipMalloc((void**)&d.frob, frob.size() * sizeof(u32));
    if (e == hipSuccess) e = hipMemcpy(d.prog, prog.data(), prog.size() * sizeof(u32), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d.frob, frob.data(), frob.size() * sizeof(u32), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d.prog);
        (void)hipFree(d.frob);
        return e;
    }
    d.nprog = (int)prog.size();
    *out = &(g_dev[device] = d);
    return hipSuccess;
}

hipError_t take_workspace(Workspace* w, int device) {
    {
        std::lock_guard<std::mutex> lk(g_mu);
        PerDevice* d = nullptr;
        const hipError_t e = per_device(&d, device);
        if (e != hipSuccess) return e;
        if (!d->idle.empty()) {
            *w = d->idle.back();
            d->idle.pop_back();
            return hipSuccess;
        }
    }
    Workspace n;
    hipError_t e = hipStreamCreateWithFlags(&n.st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&n.pts, 2 * SLICE * sizeof(blst_p1));
    if (e == hipSuccess) e = hipMalloc((void**)&n.ok, SLICE);
    if (e != hipSuccess) {
        if (n.st) (void)hipStreamDestroy(n.st);
        (void)hipFree(n.pts);
        (void)hipFree(n.ok);
        return e;
    }
    *w = n;
    return hipSuccess;
}
void give_workspace(const Workspace& w, int device) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_dev[device].idle.push_back(w);
}
}  // namespace

namespace kzgamd {
namespace pairing_gpu {

hipError_t device_table(DeviceTable* out, const blst_p2* q) {
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    hp::G2Jac key;
    memcpy(&key, q, sizeof key);
    {
        std::lock_guard<std::mutex> lk(g_mu);
        PerDevice* d = nullptr;  // the device's program and constants: built here, so that check_on_stream never has to
        if ((e = per_device(&d, device)) != hipSuccess) return e;
        for (const TableEntry& t : g_tables)
            if (t.device == device && memcmp(&t.key, &key, sizeof key) == 0) {
                out->words = (const u32*)t.words.get();
                out->hold = t.words;
                return hipSuccess;
            }
    }
    const std::shared_ptr<const hp::LineTable> lt = hp::prepared_lines(key);
    std::shared_ptr<void> words;
    if (!lt->inf) {
        if (lt->lambda.size() != (size_t)fp12w::LINE_STEPS || lt->c.size() != (size_t)fp12w::LINE_STEPS) return hipErrorInvalidValue;
        std::vector<u32> h(fp12w::TABLE_WORDS);
        for (int s = 0; s < fp12w::LINE_STEPS; ++s) {
            u32* w = &h[(size_t)s * fp12w::LINE_WORDS];
            put_fp(w, lt->lambda[s].c0);
            put_fp(w + 16, lt->lambda[s].c1);
            put_fp(w + 32, lt->c[s].c0);
            put_fp(w + 48, lt->c[s].c1);
        }
        void* d = nullptr;
        e = hipMalloc(&d, h.size() * sizeof(u32));
        if (e != hipSuccess) return e;
        words = std::shared_ptr<void>(d, HipFree());
        e = hipMemcpy(d, h.data(), h.size() * sizeof(u32), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    for (const TableEntry& t : g_tables)  // another thread built the same table meanwhile: its entry is the one that stays
        if (t.device == device && memcmp(&t.key, &key, sizeof key) == 0) {
            out->words = (const u32*)t.words.get();
            out->hold = t.words;
            return hipSuccess;
        }
    if (g_tables.size() >= 16) g_tables.erase(g_tables.begin());
    g_tables.push_back({device, key, words});
    out->words = (const u32*)words.get();
    out->hold = words;
    return hipSuccess;
}

hipError_t check_on_stream(uint8_t* ok, const blst_p1* a1, const blst_p1* b1, const DeviceTable& ta, const DeviceTable& tb,
                           size_t count, hipStream_t st) {
    if (count == 0) return hipSuccess;
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    PerDevice* d = nullptr;
    u32 *prog, *frob;
    int nprog;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        e = per_device(&d, device);
        if (e != hipSuccess) return e;
        prog = d->prog, frob = d->frob, nprog = d->nprog;
    }
    for (size_t at = 0; at < count; at += 1u << 20) {  // the grid stays far below the launch limit
        const size_t n = count - at < (1u << 20) ? count - at : (1u << 20);
        hipLaunchKernelGGL(k_pairing_check, dim3((unsigned)n), dim3(64), 0, st, ok + at, a1 + at, b1 + at, ta.words, tb.words,
                           (const u32*)prog, nprog, (const u32*)frob, (unsigned)n);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace pairing_gpu
}  // namespace kzgamd

extern "C" int kzgamd_pairing_info(size_t* slice_checks) {
    if (slice_checks) *slice_checks = SLICE;
    return 0;
}

extern "C" int kzgamd_pairings_verify_batch(bool* ok, const blst_p1* a1, const blst_p2* a2, const blst_p1* b1, const blst_p2* b2,
                                            size_t count) {
    if (count == 0) return 0;
    if (!ok || !a1 || !a2 || !b1 || !b2) return -1;
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return kzgamd::dev_code(e);
    try {
        DeviceTable ta, tb;
        if ((e = kzgamd::pairing_gpu::device_table(&ta, a2)) != hipSuccess) return kzgamd::dev_code(e);
        if ((e = kzgamd::pairing_gpu::device_table(&tb, b2)) != hipSuccess) return kzgamd::dev_code(e);
        std::vector<uint8_t> verdicts(count < SLICE ? count : SLICE);  // before the workspace: nothing below throws
        Workspace w;
        if ((e = take_workspace(&w, device)) != hipSuccess) return kzgamd::dev_code(e);
        for (size_t at = 0; at < count && e == hipSuccess; at += SLICE) {
            const size_t n = count - at < SLICE ? count - at : SLICE;
            e = hipMemcpyAsync(w.pts, a1 + at, n * sizeof(blst_p1), hipMemcpyHostToDevice, w.st);
            if (e == hipSuccess) e = hipMemcpyAsync(w.pts + SLICE, b1 + at, n * sizeof(blst_p1), hipMemcpyHostToDevice, w.st);
            if (e == hipSuccess) e = kzgamd::pairing_gpu::check_on_stream(w.ok, w.pts, w.pts + SLICE, ta, tb, n, w.st);
            if (e == hipSuccess) e = hipMemcpyAsync(verdicts.data(), w.ok, n, hipMemcpyDeviceToHost, w.st);
            const hipError_t es = hipStreamSynchronize(w.st);  // also after an error: a copy may be in flight
            if (e == hipSuccess) e = es;
            if (e == hipSuccess)
                for (size_t i = 0; i < n; ++i) ok[at + i] = verdicts[i] != 0;
        }
        give_workspace(w, device);
        return e == hipSuccess ? 0 : kzgamd::dev_code(e);
    } catch (...) {
        return -2;
    }
}
