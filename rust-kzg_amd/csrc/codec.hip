// Batched point serialisation: G1::from_bytes / to_bytes / is_valid, G2::from_bytes / to_bytes and
// G1Affine::into_affines of the reference (kzg/src/lib.rs:89-99, 400-402, 255-265) for many points in one call.
//     kzgamd_g1_compress_batch / kzgamd_g1_to_affine_batch    Jacobian blst_p1 -> 48 bytes / blst_p1_affine
//     kzgamd_g1_uncompress_batch                              48 bytes -> blst_p1, with the subgroup test on request
//     kzgamd_g2_compress_batch / kzgamd_g2_uncompress_batch   the same for blst_p2 and 96 bytes
//
// Handle-less, as groupmul.hip: host buffers, the calling thread's device (or cfg->device), a stream per call, one slice
// of workspace that larger counts run through.  Everything runs on the GPU for every n >= 1.
//
// G1 in: the decode kernels of the c-kzg surface (ckz::decode_enqueue: four points per wave up to WIDE_CHECK_MAX points
// of a slice, a lane per point above) and k_affpt_to_blst_p1.  G1 out: a lane per chunk of 1, 4 or 8 points by the count,
// one inversion per lane (g1io::jac_chunk_out).  G2: a lane per point both ways (g2_io.hip.h); one-wave workgroups, no barrier.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/kzg_mi355x.h"
#include "ckzg_shared.h"
#include "config.h"
#include "device_guard.h"
#include "g1_io.hip.h"
#include "g2_io.hip.h"
#include "host_call.h"

using kzgamd::blocks;
using kzgamd::ScopedBuf;

namespace {

constexpr size_t SLICE_DEFAULT = (size_t)1 << 18;  // points per slice: at most 75 MB of blst_p2 and 25 MB of bytes
constexpr size_t SLICE_MIN = 64;
// points per lane of k_g1_jac_out by the count of a launch, each the fastest measured (profiles/NOTES.md, section 39):
// one up to G1_CHUNK1_MAX points (the chip is not full: the shortest chain wins), four up to G1_CHUNK4_MAX, eight above
constexpr size_t G1_CHUNK1_MAX = (size_t)1 << 16, G1_CHUNK4_MAX = (size_t)1 << 18;

// lane t: the points [t * CH, (t + 1) * CH) of `in` (blst_p1 layout) -> 48 bytes each, or blst_p1_affine
template <int CH, bool AFFINE>
__global__ void __launch_bounds__(64) k_g1_jac_out(void* __restrict__ out, const ff::Fp* __restrict__ in, size_t n) {
    const size_t at = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * CH;
    if (at >= n) return;
    const int m = n - at < (size_t)CH ? (int)(n - at) : CH;
    g1io::jac_chunk_out<CH, AFFINE>((unsigned char*)out + at * (AFFINE ? 96 : 48), in + 3 * at, m);
}

// 96 bytes -> blst_p2 (Z = one; infinity and every refused point all-zero) + status: 0 ok, 1 not a valid encoding,
// 2 (CHECK) on the twist but outside G2
template <bool CHECK>
__global__ void __launch_bounds__(64) k_g2_decode(ff::Fp* __restrict__ out, int* __restrict__ status,
                                                  const unsigned char* __restrict__ in, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned char buf[96];
    for (int k = 0; k < 96; ++k) buf[k] = in[96 * i + k];
    g2::AffPt p;
    int st = g2io::uncompress(p, buf) ? 0 : 1;
    if (CHECK && st == 0 && !g2io::in_g2(p)) st = 2;
    status[i] = st;
    ff::Fp* o = out + 6 * i;
    if (st != 0 || (p.flags & 1)) {
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = ff::Fp::zero();
        return;
    }
    g2::to_blst(o, p.x);
    g2::to_blst(o + 2, p.y);
    o[4] = ff::Fp::one();
    o[5] = ff::Fp::zero();
}

// blst_p2 (any Z; Z all-zero: the identity) -> 96 bytes
__global__ void __launch_bounds__(64) k_g2_compress(unsigned char* __restrict__ out, const ff::Fp* __restrict__ in, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    g2::Jac p;
    g2::from_blst_jacobian(p, in + 6 * i);
    unsigned char buf[96];
    g2io::compress(buf, p);
    for (int k = 0; k < 96; ++k) out[96 * i + k] = buf[k];
}

template <int CH, bool AFFINE>
void launch_g1_jac_out(void* d_out, const void* d_in, size_t cnt, hipStream_t st) {
    hipLaunchKernelGGL((k_g1_jac_out<CH, AFFINE>), dim3(blocks((cnt + CH - 1) / CH, 64)), dim3(64), 0, st, d_out, (const ff::Fp*)d_in, cnt);
}
template <bool AFFINE>
void enqueue_g1_jac_out(void* d_out, const void* d_in, size_t cnt, hipStream_t st) {
    if (cnt <= G1_CHUNK1_MAX) launch_g1_jac_out<1, AFFINE>(d_out, d_in, cnt, st);
    else if (cnt <= G1_CHUNK4_MAX) launch_g1_jac_out<4, AFFINE>(d_out, d_in, cnt, st);
    else launch_g1_jac_out<8, AFFINE>(d_out, d_in, cnt, st);
}

using Stream = kzgamd::CallStream;

// what a KzgAmdConfig means to these calls: 0, or the call's return code
int read_config(const KzgAmdConfig* cfg, const char* who, int* device, size_t* slice) {
    return kzgamd::read_slice_config(cfg, who, "codec_slice", SLICE_DEFAULT, SLICE_MIN, device, slice);
}

// the frame of every call: the device, a stream, then body(stream, slice) with slice <= n
template <class F>
int run(const KzgAmdConfig* cfg, const char* who, size_t n, F&& body) {
    int device;
    size_t slice;
    if (int rc = read_config(cfg, who, &device, &slice)) return rc;
    return kzgamd::status_of([&]() -> int {
        if (device < 0) DEV_TRY(hipGetDevice(&device));
        kzgamd::DeviceGuard on_device(device);
        DEV_TRY(on_device.err);
        Stream s;
        return body(s.st, slice > n ? n : slice);
    });
}

// out[at .. at + cnt) of `out_size` bytes each from in[at .. at + cnt) of `in_size` bytes each, slice by slice
template <class Enqueue>
int convert(const KzgAmdConfig* cfg, const char* who, void* out, size_t out_size, const void* in, size_t in_size, size_t n,
            Enqueue&& enqueue) {
    return run(cfg, who, n, [&](hipStream_t st, size_t slice) -> int {
        ScopedBuf d_in, d_out;
        d_in.alloc(slice * in_size);
        d_out.alloc(slice * out_size);
        for (size_t at = 0; at < n; at += slice) {
            const size_t cnt = n - at < slice ? n - at : slice;
            DEV_TRY(hipMemcpyAsync(d_in.p, (const char*)in + at * in_size, cnt * in_size, hipMemcpyHostToDevice, st));
            enqueue(d_out.p, d_in.p, cnt, st);
            DEV_TRY(hipGetLastError());
            DEV_TRY(hipMemcpyAsync((char*)out + at * out_size, d_out.p, cnt * out_size, hipMemcpyDeviceToHost, st));
            DEV_TRY(hipStreamSynchronize(st));
        }
        return 0;
    });
}

// the two parsers: as convert, with a status per point; refused entries are zeroed here, on the way out
template <class Enqueue>
int parse(const KzgAmdConfig* cfg, const char* who, void* out, size_t out_size, uint8_t* status, const void* in, size_t in_size,
          size_t n, size_t work_size, Enqueue&& enqueue) {
    return run(cfg, who, n, [&](hipStream_t st, size_t slice) -> int {
        ScopedBuf d_in, d_out, d_stat, d_work;
        d_in.alloc(slice * in_size);
        d_out.alloc(slice * out_size);
        d_stat.alloc(slice * sizeof(int));
        d_work.alloc(slice * work_size);
        std::vector<int> stat(slice);
        int refused = 0;
        for (size_t at = 0; at < n; at += slice) {
            const size_t cnt = n - at < slice ? n - at : slice;
            DEV_TRY(hipMemcpyAsync(d_in.p, (const char*)in + at * in_size, cnt * in_size, hipMemcpyHostToDevice, st));
            DEV_TRY(hipMemsetAsync(d_stat.p, 0, cnt * sizeof(int), st));
            if (work_size) DEV_TRY(hipMemsetAsync(d_work.p, 0, cnt * work_size, st));
            enqueue(d_out.p, (int*)d_stat.p, d_work.p, d_in.p, cnt, st);
            DEV_TRY(hipGetLastError());
            DEV_TRY(hipMemcpyAsync((char*)out + at * out_size, d_out.p, cnt * out_size, hipMemcpyDeviceToHost, st));
            DEV_TRY(hipMemcpyAsync(stat.data(), d_stat.p, cnt * sizeof(int), hipMemcpyDeviceToHost, st));
            DEV_TRY(hipStreamSynchronize(st));
            for (size_t i = 0; i < cnt; ++i) {
                if (stat[i]) {
                    refused = 1;
                    memset((char*)out + (at + i) * out_size, 0, out_size);
                }
                if (status) status[at + i] = (uint8_t)stat[i];
            }
        }
        return refused;
    });
}

}  // namespace

extern "C" int kzgamd_codec_info(size_t* slice_points) {
    if (slice_points) *slice_points = SLICE_DEFAULT;
    return 0;
}

extern "C" int kzgamd_g1_compress_batch(uint8_t* out48, const blst_p1* in, size_t n, const KzgAmdConfig* cfg) {
    if (n == 0) return 0;
    if (!out48 || !in) return -1;
    return convert(cfg, "kzgamd_g1_compress_batch", out48, 48, in, sizeof(blst_p1), n, enqueue_g1_jac_out<false>);
}

extern "C" int kzgamd_g1_to_affine_batch(blst_p1_affine* out, const blst_p1* in, size_t n, const KzgAmdConfig* cfg) {
    if (n == 0) return 0;
    if (!out || !in) return -1;
    return convert(cfg, "kzgamd_g1_to_affine_batch", out, sizeof(blst_p1_affine), in, sizeof(blst_p1), n, enqueue_g1_jac_out<true>);
}

extern "C" int kzgamd_g1_uncompress_batch(blst_p1* out, uint8_t* status, const uint8_t* in48, size_t n, int check_subgroup,
                                          const KzgAmdConfig* cfg) {
    if (n == 0) return 0;
    if (!out || !in48) return -1;
    const bool check = check_subgroup != 0;
    return parse(cfg, "kzgamd_g1_uncompress_batch", out, sizeof(blst_p1), status, in48, 48, n, sizeof(g1::AffPt),
                 [check](void* d_out, int* d_stat, void* d_slots, const void* d_in, size_t cnt, hipStream_t st) {
                     ckz::decode_enqueue((g1::AffPt*)d_slots, d_stat, (const unsigned char*)d_in, cnt, st, check);
                     ckz::affpt_to_blst_p1_enqueue(d_out, (const g1::AffPt*)d_slots, cnt, st);
                 });
}

extern "C" int kzgamd_g2_compress_batch(uint8_t* out96, const blst_p2* in, size_t n, const KzgAmdConfig* cfg) {
    if (n == 0) return 0;
    if (!out96 || !in) return -1;
    return convert(cfg, "kzgamd_g2_compress_batch", out96, 96, in, sizeof(blst_p2), n, [](void* d_out, const void* d_in, size_t cnt, hipStream_t st) {
        hipLaunchKernelGGL(k_g2_compress, dim3(blocks(cnt, 64)), dim3(64), 0, st, (unsigned char*)d_out, (const ff::Fp*)d_in, cnt);
    });
}

extern "C" int kzgamd_g2_uncompress_batch(blst_p2* out, uint8_t* status, const uint8_t* in96, size_t n, int check_subgroup,
                                          const KzgAmdConfig* cfg) {
    if (n == 0) return 0;
    if (!out || !in96) return -1;
    const bool check = check_subgroup != 0;
    return parse(cfg, "kzgamd_g2_uncompress_batch", out, sizeof(blst_p2), status, in96, 96, n, 0,
                 [check](void* d_out, int* d_stat, void*, const void* d_in, size_t cnt, hipStream_t st) {
                     if (check)
                         hipLaunchKernelGGL(k_g2_decode<true>, dim3(blocks(cnt, 64)), dim3(64), 0, st, (ff::Fp*)d_out, d_stat,
                                            (const unsigned char*)d_in, cnt);
                     else
                         hipLaunchKernelGGL(k_g2_decode<false>, dim3(blocks(cnt, 64)), dim3(64), 0, st, (ff::Fp*)d_out, d_stat,
                                            (const unsigned char*)d_in, cnt);
                 });
}

// ---------------------------------------------------------------- setup files of any size: host text around the calls above
// The layout load_trusted_setup_file reads: the two counts, the Lagrange G1 points in natural order, the G2 points, the
// monomial G1 points; lowercase hex, one point per line, lines joined by '\n' (none after the last).
namespace {

void put_hex_lines(std::string& text, const std::vector<uint8_t>& bytes, size_t width) {
    static const char digits[] = "0123456789abcdef";
    for (size_t i = 0; i < bytes.size(); ++i) {
        if (i % width == 0) text += '\n';
        text += digits[bytes[i] >> 4];
        text += digits[bytes[i] & 15];
    }
}

// the next count * width bytes of the text, as ckz::scan_hex_byte reads them (into `out` unless it is NULL)
bool scan_bytes(const std::string& text, size_t& off, size_t total, std::vector<uint8_t>* out) {
    if (out) out->resize(total);
    uint8_t b;
    for (size_t i = 0; i < total; ++i) {
        if (!ckz::scan_hex_byte(text, off, b)) return false;
        if (out) (*out)[i] = b;
    }
    return true;
}

}  // namespace

extern "C" int kzgamd_write_trusted_setup_file(FILE* out, const blst_p1* g1_monomial, const blst_p1* g1_lagrange,
                                               const blst_p2* g2_monomial, size_t num_g1, size_t num_g2, const KzgAmdConfig* cfg) {
    if (!out || (num_g1 && (!g1_monomial || !g1_lagrange)) || (num_g2 && !g2_monomial)) return -1;
    try {
        std::vector<uint8_t> lag(48 * num_g1), mono(48 * num_g1), g2(96 * num_g2);
        if (int rc = kzgamd_g1_compress_batch(lag.data(), g1_lagrange, num_g1, cfg)) return rc;
        if (int rc = kzgamd_g2_compress_batch(g2.data(), g2_monomial, num_g2, cfg)) return rc;
        if (int rc = kzgamd_g1_compress_batch(mono.data(), g1_monomial, num_g1, cfg)) return rc;
        std::string text = std::to_string(num_g1) + "\n" + std::to_string(num_g2);
        text.reserve(text.size() + 97 * 2 * num_g1 + 193 * num_g2);
        put_hex_lines(text, lag, 48);
        put_hex_lines(text, g2, 96);
        put_hex_lines(text, mono, 48);
        if (fwrite(text.data(), 1, text.size(), out) != text.size() || fflush(out) != 0) return -2;
        return 0;
    } catch (...) {
        return -2;
    }
}

extern "C" int kzgamd_read_trusted_setup_file(FILE* in, blst_p1* g1_monomial, blst_p1* g1_lagrange, blst_p2* g2_monomial,
                                              size_t* num_g1, size_t* num_g2, const KzgAmdConfig* cfg) {
    if (!in || !num_g1 || !num_g2) return -1;
    try {
        std::string text;
        char chunk[1 << 16];
        for (size_t got; (got = fread(chunk, 1, sizeof chunk, in)) > 0;) text.append(chunk, got);
        const size_t cap1 = *num_g1, cap2 = *num_g2;
        size_t off = 0, n1 = 0, n2 = 0;
        if (!ckz::scan_number(text, off, n1) || !ckz::scan_number(text, off, n2)) return 1;
        // every byte takes at least one character of text: counts the text cannot hold are malformed, not allocated
        if (n1 > text.size() || n2 > text.size() || 96 * n1 + 96 * n2 > text.size() - off) return 1;
        *num_g1 = n1;
        *num_g2 = n2;
        if (((g1_monomial || g1_lagrange) && n1 > cap1) || (g2_monomial && n2 > cap2)) return 2;
        std::vector<uint8_t> lag, g2, mono;
        if (!scan_bytes(text, off, 48 * n1, g1_lagrange ? &lag : nullptr) || !scan_bytes(text, off, 96 * n2, g2_monomial ? &g2 : nullptr) ||
            !scan_bytes(text, off, 48 * n1, g1_monomial ? &mono : nullptr))
            return 1;
        int refused = 0;
        if (g1_lagrange) {
            const int rc = kzgamd_g1_uncompress_batch(g1_lagrange, nullptr, lag.data(), n1, 1, cfg);
            if (rc < 0) return rc;
            refused |= rc;
        }
        if (g2_monomial) {
            const int rc = kzgamd_g2_uncompress_batch(g2_monomial, nullptr, g2.data(), n2, 1, cfg);
            if (rc < 0) return rc;
            refused |= rc;
        }
        if (g1_monomial) {
            const int rc = kzgamd_g1_uncompress_batch(g1_monomial, nullptr, mono.data(), n1, 1, cfg);
            if (rc < 0) return rc;
            refused |= rc;
        }
        return refused ? 3 : 0;
    } catch (...) {
        return -2;
    }
}
