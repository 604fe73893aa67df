// The pairing tower Fp2 / Fp6 / Fp12 over the lane-parallel Fp of fpw.hip.h, one wave per value: a coefficient is one
// register (limb i in lane i of a DPP row), replicated in the four rows as g1w keeps its points, and the independent Fp
// products of a tower operation run four per wmul4 step (wmuln).  host_pairing.h is the specification: the same tower,
// the same Karatsuba splits, the same Granger-Scott squaring, the same sparse line product, the same final
// exponentiation chain, operation for operation; only f2_sqr inside f6_inv is taken as f2_mul(a, a), so that every Fp2
// product goes through one batch routine.
//
// Forms (all with lanes 14 and 15 zero and the four rows identical):
//   N-form   limbs 0..12 <= 2^28 (what wnorm returns), the value given per routine as a multiple of p
//   R-form   N-form with value < 2p: what every operation of the interpreter (run_program) takes and returns
// Products: wmul4 is exact Montgomery — for operands with limbs <= 2^29 it returns (a*b + m*p) / 2^392 with m < 2^392,
// N-form, value < a*b / 2^392 + p.  fpw.hip.h states the case a*b < 2^392 * p = 2520 p^2 (value < 2p); the same chain
// holds beyond it as long as the accumulator fits (values up to ~1000p: acc < 2a + 2p, top limb < 2^29), and that is what
// the reduction at the end of every operation uses: x * (2^392 mod p) leaves x mod p and brings a value < 2520p under 2p.
// Subtractions (wsubk<K>) add K*p with three units borrowed into each limb: the subtrahend may be the LAZY sum of two
// N-form values (limbs <= 2^29 <= 3 * (2^28 - 1)), its value at most (K-1)p; the result is N-form, value < a + K*p.
// The lazy sums of Karatsuba only ever add two N-form values (limbs <= 2^29), every other sum is normalized (waddn).
//
// Values live in LDS between operations (a slot is 12 coefficients x 16 limbs, 768 bytes, in words THAT BELONG TO THE
// CALLING WAVE); an operation loads its operands into registers, works there, and stores the result.  One interpreter
// loop (run_program) holds the body of every operation once: the Miller loop and the final exponentiation are a few
// hundred instruction words, built on the host (pairing.hip), and the device harness of the tests runs the same
// bodies on single operations.
#pragma once
#include "fpw.hip.h"
#include "g1w.hip.h"

namespace fp12w {
using ff::u32;
using ff::u64;

constexpr int SLOT_WORDS = 12 * 16;   // one Fp12 in LDS
constexpr int NSLOTS = 10;            // what the pairing program uses
constexpr int FP_WORDS = 16;          // one Fp in LDS
constexpr int PAIR_WORDS = 3 * FP_WORDS;                   // per pair: Z^3, X*Z, Y (sign applied)
constexpr int WAVE_WORDS = NSLOTS * SLOT_WORDS + 2 * PAIR_WORDS + 16;  // + 16 words of exchange scratch
constexpr int LINE_STEPS = 68;        // 63 doublings + 5 additions
constexpr int LINE_WORDS = 4 * 16;    // per step: lambda.c0, lambda.c1, c.c0, c.c1, canonical fp28 limbs, 16 words each
constexpr int TABLE_WORDS = LINE_STEPS * LINE_WORDS;
constexpr int FROB_WORDS = 12 * 16;   // g[0..5] as Fp2, canonical fp28 limbs

// instruction word: op | d << 8 | a << 16 | b << 24
enum Op : u32 { OP_END = 0, OP_ONE, OP_MUL, OP_SQR, OP_CSQR, OP_CONJ, OP_FROB, OP_INV, OP_LINE };
constexpr u32 insn(u32 op, u32 d, u32 a, u32 b = 0) { return op | d << 8 | a << 16 | b << 24; }

struct Ctx {
    fpw::Lane lc;
    u32 one;                        // this lane's limb of 2^392 mod p
    u32 p8, p32, p64, p128, p512;   // this lane's limb of K*p, three units borrowed into each of the limbs 0..12
    int lane, row, li;
};

template <int K>
__device__ __forceinline__ u32 padk_limb(int li) {
    constexpr fp28::PadW w = fp28::padw<K, 3>();
    constexpr u32 T[16] = {w.v[0], w.v[1], w.v[2], w.v[3], w.v[4], w.v[5], w.v[6], w.v[7],
                           w.v[8], w.v[9], w.v[10], w.v[11], w.v[12], w.v[13], 0u, 0u};
    return T[li];
}
__device__ __forceinline__ Ctx make_ctx(int lane) {
    constexpr u32 ONE[16] = {fp28::one_l(0), fp28::one_l(1), fp28::one_l(2),  fp28::one_l(3),  fp28::one_l(4),  fp28::one_l(5),
                             fp28::one_l(6), fp28::one_l(7), fp28::one_l(8),  fp28::one_l(9),  fp28::one_l(10), fp28::one_l(11),
                             fp28::one_l(12), fp28::one_l(13), 0u, 0u};
    Ctx c;
    c.lc = fpw::lane_consts(lane);
    c.lane = lane;
    c.row = lane >> 4;
    c.li = lane & 15;
    c.one = ONE[c.li];
    c.p8 = padk_limb<8>(c.li);
    c.p32 = padk_limb<32>(c.li);
    c.p64 = padk_limb<64>(c.li);
    c.p128 = padk_limb<128>(c.li);
    c.p512 = padk_limb<512>(c.li);
    return c;
}
template <int K>
__device__ __forceinline__ u32 padk(const Ctx& c) {
    static_assert(K == 8 || K == 32 || K == 64 || K == 128 || K == 512, "pad multiple");
    return K == 8 ? c.p8 : K == 32 ? c.p32 : K == 64 ? c.p64 : K == 128 ? c.p128 : c.p512;
}

// ---------------------------------------------------------------- Fp
// a + b: N-form in (or one of them a lazy sum, limbs < 2^31 in all), N-form out
__device__ __forceinline__ u32 waddn(u32 a, u32 b, const Ctx& c) { return fpw::wnorm(a + b, c.lc); }
// a + K*p - b.  a: limbs <= 2^29; b: limbs 0..12 <= 3 * 2^28 - 3, value <= (K-1)p.  N-form, value < a + K*p
template <int K>
__device__ __forceinline__ u32 wsubk(u32 a, u32 b, const Ctx& c) { return fpw::wnorm(a + padk<K>(c) - b, c.lc); }
// 8p - a for an N-form a <= 7p: N-form, value <= 8p
__device__ __forceinline__ u32 wneg8(u32 a, const Ctx& c) { return wsubk<8>(0u, a, c); }

// r[k] = a[k] * b[k] * 2^-392, N products four at a time in the rows of the wave.  Operands: limbs <= 2^29, lanes 14 and 15
// zero, the rows identical; results: N-form, value < a*b / 2^392 + p, the rows identical.
template <int N>
__device__ __forceinline__ void wmuln(u32 (&r)[N], const u32 (&a)[N], const u32 (&b)[N], const Ctx& c) {
#pragma unroll
    for (int j = 0; j < N; j += 4) {
        const int j1 = j + 1 < N ? j + 1 : N - 1, j2 = j + 2 < N ? j + 2 : N - 1, j3 = j + 3 < N ? j + 3 : N - 1;
        const u32 t = fpw::wmul4(fpw::rows4(c.row, a[j], a[j1], a[j2], a[j3]), fpw::rows4(c.row, b[j], b[j1], b[j2], b[j3]), c.lc);
        r[j] = fpw::row_all(t, 0, c.lane);
        if (j + 1 < N) r[j + 1] = fpw::row_all(t, 1, c.lane);
        if (j + 2 < N) r[j + 2] = fpw::row_all(t, 2, c.lane);
        if (j + 3 < N) r[j + 3] = fpw::row_all(t, 3, c.lane);
    }
}
// x * (2^392 mod p) * 2^-392: the same residue, R-form, for N-form values < 2520p
template <int N>
__device__ __forceinline__ void wreduce(u32 (&x)[N], const Ctx& c) {
    u32 o[N], r[N];
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = c.one;
    wmuln<N>(r, x, o, c);
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = r[k];
}
// a^(p-2), 4-bit windows as k_decode_g1_wide's square root: 14 table products, then 4 squarings and at most one product
// per nibble.  a: N-form, value < 50p; R-form out (0 for a = 0 mod p).
__device__ __forceinline__ u32 pm2_nibble(int j) {
    constexpr u32 E[12] = {0xffffaaa9u, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u,
                           0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau};  // p - 2
    return (E[j >> 3] >> (4 * (j & 7))) & 15u;
}
__device__ __forceinline__ u32 winv(u32 a, const Ctx& c) {
    u32 t[16];
    t[0] = 0;
    t[1] = fpw::wmul4(a, c.one, c.lc);
#pragma unroll
    for (int k = 2; k < 16; ++k) t[k] = fpw::wmul4(t[k - 1], t[1], c.lc);
    auto pick = [&](u32 d) -> u32 {
        u32 v = t[1];
#pragma unroll
        for (int k = 2; k < 16; ++k) {
            v = d == (u32)k ? t[k] : v;
            asm("" : "+v"(v));  // a chain of selects, not a table on the stack indexed by d
        }
        return v;
    };
    u32 acc = t[1];  // the top nibble of p - 2 is 1
#pragma unroll 1
    for (int j = 94; j >= 0; --j) {
#pragma unroll 1
        for (int q = 0; q < 4; ++q) acc = fpw::wmul4(acc, acc, c.lc);
        const u32 d = pm2_nibble(j);
        if (d) acc = fpw::wmul4(acc, pick(d), c.lc);
    }
    return acc;
}

// ---------------------------------------------------------------- Fp2
struct F2 {
    u32 c0, c1;
};
__device__ __forceinline__ F2 f2_addn(const F2& a, const F2& b, const Ctx& c) { return {waddn(a.c0, b.c0, c), waddn(a.c1, b.c1, c)}; }
__device__ __forceinline__ F2 f2_addl(const F2& a, const F2& b) { return {a.c0 + b.c0, a.c1 + b.c1}; }  // lazy: N-form operands only
template <int K>
__device__ __forceinline__ F2 f2_sub(const F2& a, const F2& b, const Ctx& c) { return {wsubk<K>(a.c0, b.c0, c), wsubk<K>(a.c1, b.c1, c)}; }
// a * (1 + u) = (a0 - a1, a0 + a1): a N-form, a.c1 <= (K-1)p; result < a0 + K*p, a0 + a1
template <int K>
__device__ __forceinline__ F2 f2_mul_xi(const F2& a, const Ctx& c) { return {wsubk<K>(a.c0, a.c1, c), waddn(a.c0, a.c1, c)}; }
// N Karatsuba products side by side: 3N Fp products.  Coefficients N-form with (a0 + a1) * (b0 + b1) < 2520 p^2 (every Fp
// product then < 2p); results N-form, value < 10p.
template <int N>
__device__ __forceinline__ void f2_muln(F2 (&r)[N], const F2 (&a)[N], const F2 (&b)[N], const Ctx& c) {
    u32 x[3 * N], y[3 * N], t[3 * N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        x[3 * k] = a[k].c0;
        y[3 * k] = b[k].c0;
        x[3 * k + 1] = a[k].c1;
        y[3 * k + 1] = b[k].c1;
        x[3 * k + 2] = a[k].c0 + a[k].c1;  // lazy, limbs <= 2^29
        y[3 * k + 2] = b[k].c0 + b[k].c1;
    }
    wmuln<3 * N>(t, x, y, c);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        r[k].c0 = wsubk<8>(t[3 * k], t[3 * k + 1], c);
        r[k].c1 = wsubk<8>(t[3 * k + 2], t[3 * k] + t[3 * k + 1], c);
    }
}

// ---------------------------------------------------------------- Fp6
struct F6 {
    F2 c0, c1, c2;
};
__device__ __forceinline__ F6 f6_addn(const F6& a, const F6& b, const Ctx& c) { return {f2_addn(a.c0, b.c0, c), f2_addn(a.c1, b.c1, c), f2_addn(a.c2, b.c2, c)}; }
__device__ __forceinline__ F6 f6_addl(const F6& a, const F6& b) { return {f2_addl(a.c0, b.c0), f2_addl(a.c1, b.c1), f2_addl(a.c2, b.c2)}; }
template <int K>
__device__ __forceinline__ F6 f6_sub(const F6& a, const F6& b, const Ctx& c) { return {f2_sub<K>(a.c0, b.c0, c), f2_sub<K>(a.c1, b.c1, c), f2_sub<K>(a.c2, b.c2, c)}; }
template <int K>
__device__ __forceinline__ F6 f6_mul_v(const F6& a, const Ctx& c) { return {f2_mul_xi<K>(a.c2, c), a.c0, a.c1}; }
// the six operand pairs of the Karatsuba product a * b (coefficient sums normalized) ...
__device__ __forceinline__ void f6_mul_pre(F2* x, F2* y, const F6& a, const F6& b, const Ctx& c) {
    x[0] = a.c0, y[0] = b.c0;
    x[1] = a.c1, y[1] = b.c1;
    x[2] = a.c2, y[2] = b.c2;
    x[3] = f2_addn(a.c1, a.c2, c), y[3] = f2_addn(b.c1, b.c2, c);
    x[4] = f2_addn(a.c0, a.c1, c), y[4] = f2_addn(b.c0, b.c1, c);
    x[5] = f2_addn(a.c0, a.c2, c), y[5] = f2_addn(b.c0, b.c2, c);
}
// ... and the product from their six Fp2 products (< 10p each): N-form, c0 < 116p, c1 < 84p, c2 < 52p
__device__ __forceinline__ F6 f6_mul_post(const F2* t, const Ctx& c) {
    const F2 s12 = f2_sub<32>(t[3], f2_addl(t[1], t[2]), c);  // < 42p
    const F2 s01 = f2_sub<32>(t[4], f2_addl(t[0], t[1]), c);
    const F2 s02 = f2_sub<32>(t[5], f2_addl(t[0], t[2]), c);
    return {f2_addn(t[0], f2_mul_xi<64>(s12, c), c), f2_addn(s01, f2_mul_xi<32>(t[2], c), c), f2_addn(s02, t[1], c)};
}

// ---------------------------------------------------------------- Fp12
struct F12 {
    F6 c0, c1;
};
__device__ __forceinline__ void f12_to_arr(u32 (&v)[12], const F12& a) {
    v[0] = a.c0.c0.c0, v[1] = a.c0.c0.c1, v[2] = a.c0.c1.c0, v[3] = a.c0.c1.c1, v[4] = a.c0.c2.c0, v[5] = a.c0.c2.c1;
    v[6] = a.c1.c0.c0, v[7] = a.c1.c0.c1, v[8] = a.c1.c1.c0, v[9] = a.c1.c1.c1, v[10] = a.c1.c2.c0, v[11] = a.c1.c2.c1;
}
__device__ __forceinline__ F12 f12_from_arr(const u32 (&v)[12]) {
    return {{{v[0], v[1]}, {v[2], v[3]}, {v[4], v[5]}}, {{v[6], v[7]}, {v[8], v[9]}, {v[10], v[11]}}};
}
// N-form coefficients < 2520p -> R-form
__device__ __forceinline__ F12 f12_reduce(const F12& a, const Ctx& c) {
    u32 v[12];
    f12_to_arr(v, a);
    wreduce<12>(v, c);
    return f12_from_arr(v);
}
__device__ __forceinline__ F6 f6_reduce(const F6& a, const Ctx& c) {
    u32 v[6] = {a.c0.c0, a.c0.c1, a.c1.c0, a.c1.c1, a.c2.c0, a.c2.c1};
    wreduce<6>(v, c);
    return {{v[0], v[1]}, {v[2], v[3]}, {v[4], v[5]}};
}
// slot <-> registers; the first row stores, every row loads its own copy
__device__ __forceinline__ F12 f12_load(const u32* sh, u32 slot, const Ctx& c) {
    u32 v[12];
    const u32* s = sh + slot * SLOT_WORDS + c.li;
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = s[16 * k];
    return f12_from_arr(v);
}
__device__ __forceinline__ void f12_store(u32* sh, u32 slot, const F12& a, const Ctx& c) {
    u32 v[12];
    f12_to_arr(v, a);
    u32* s = sh + slot * SLOT_WORDS + c.li;
    if (c.row == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) s[16 * k] = v[k];
    }
}

// a * b: 18 Fp2 products.  R-form in (operand sums < 4p, < 8p, lazy < 16p); before the reduction c0 < 360p, c1 < 628p
__device__ __forceinline__ F12 f12_mul(const F12& a, const F12& b, const Ctx& c) {
    F2 x[18], y[18], t[18];
    f6_mul_pre(x, y, a.c0, b.c0, c);
    f6_mul_pre(x + 6, y + 6, a.c1, b.c1, c);
    f6_mul_pre(x + 12, y + 12, f6_addn(a.c0, a.c1, c), f6_addn(b.c0, b.c1, c), c);
    f2_muln<18>(t, x, y, c);
    const F6 t0 = f6_mul_post(t, c), t1 = f6_mul_post(t + 6, c), m = f6_mul_post(t + 12, c);  // < 116p
    return f12_reduce({f6_addn(t0, f6_mul_v<128>(t1, c), c), f6_sub<512>(m, f6_addl(t0, t1), c)}, c);
}
// (a + b w)^2 = (a + b)(a + v b) - ab - v ab + 2ab w: 12 Fp2 products.  R-form in: v b < 10p, a + v b < 12p, its sums
// < 24p, lazy < 48p, against (a + b) lazy < 16p; before the reduction c0 < 628p, c1 < 232p
__device__ __forceinline__ F12 f12_sqr(const F12& a, const Ctx& c) {
    F2 x[12], y[12], t[12];
    f6_mul_pre(x, y, a.c0, a.c1, c);
    f6_mul_pre(x + 6, y + 6, f6_addn(a.c0, a.c1, c), f6_addn(a.c0, f6_mul_v<8>(a.c1, c), c), c);
    f2_muln<12>(t, x, y, c);
    const F6 ab = f6_mul_post(t, c), m = f6_mul_post(t + 6, c);
    return f12_reduce({f6_sub<512>(m, f6_addl(ab, f6_mul_v<128>(ab, c)), c), f6_addn(ab, ab, c)}, c);
}
// Granger-Scott squaring in the cyclotomic subgroup: three Fp4 squarings of two Fp2 products each.  R-form in; an Fp4
// squaring gives r0 < 74p, r1 < 20p, the results 3t -+ 2z stay below 238p before the reduction
__device__ __forceinline__ F12 f12_cyclotomic_sqr(const F12& f, const Ctx& c) {
    const F2 za[3] = {f.c0.c0, f.c1.c0, f.c0.c1}, zb[3] = {f.c1.c1, f.c0.c2, f.c1.c2};  // (z0, z1), (z2, z3), (z4, z5)
    F2 x[6], y[6], t[6], r0[3], r1[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        x[2 * i] = za[i], y[2 * i] = zb[i];
        x[2 * i + 1] = f2_addn(za[i], zb[i], c);
        y[2 * i + 1] = f2_addn(za[i], f2_mul_xi<8>(zb[i], c), c);
    }
    f2_muln<6>(t, x, y, c);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r0[i] = f2_sub<64>(t[2 * i + 1], f2_addl(t[2 * i], f2_mul_xi<32>(t[2 * i], c)), c);
        r1[i] = f2_addn(t[2 * i], t[2 * i], c);
    }
    auto three_minus_two = [&](const F2& tt, const F2& z) { const F2 d = f2_sub<8>(tt, z, c); return f2_addn(f2_addn(d, d, c), tt, c); };
    auto three_plus_two = [&](const F2& tt, const F2& z) { const F2 s = f2_addn(tt, z, c); return f2_addn(f2_addn(s, s, c), tt, c); };
    F12 r;
    r.c0.c0 = three_minus_two(r0[0], za[0]);
    r.c1.c1 = three_plus_two(r1[0], zb[0]);
    r.c1.c0 = three_plus_two(f2_mul_xi<32>(r1[2], c), za[1]);
    r.c0.c2 = three_minus_two(r0[2], zb[1]);
    r.c0.c1 = three_minus_two(r0[1], za[2]);
    r.c1.c2 = three_plus_two(r1[1], zb[2]);
    return f12_reduce(r, c);
}
// x * (a2 + b2 v): five Fp2 products ...
__device__ __forceinline__ void mul_ab0_pre(F2* x, F2* y, const F6& f, const F2& a2, const F2& b2, const Ctx& c) {
    x[0] = f.c0, y[0] = a2;
    x[1] = f.c1, y[1] = b2;
    x[2] = f2_addn(f.c0, f.c1, c), y[2] = f2_addn(a2, b2, c);
    x[3] = f.c2, y[3] = b2;
    x[4] = f.c2, y[4] = a2;
}
// ... c0 < 52p, c1 < 42p, c2 < 20p
__device__ __forceinline__ F6 mul_ab0_post(const F2* t, const Ctx& c) {
    return {f2_addn(t[0], f2_mul_xi<32>(t[3], c), c), f2_sub<32>(t[2], f2_addl(t[0], t[1]), c), f2_addn(t[1], t[4], c)};
}
// f * (a + b v + cy v w), the line value: f R-form, a < 2p, b and cy N-form <= 8p (a2 + bc lazy <= 36p against lazy
// < 16p).  Ten Fp2 products and six Fp products; before the reduction c0 < 62p, c1 < 116p
__device__ __forceinline__ F12 f12_mul_line(const F12& f, const F2& a, const F2& b, u32 cy, const Ctx& c) {
    F2 x[10], y[10], t[10];
    const F2 bc = {waddn(b.c0, cy, c), b.c1};
    mul_ab0_pre(x, y, f.c0, a, b, c);
    mul_ab0_pre(x + 5, y + 5, f6_addn(f.c0, f.c1, c), a, bc, c);
    f2_muln<10>(t, x, y, c);
    const F6 t0 = mul_ab0_post(t, c), m = mul_ab0_post(t + 5, c);
    // f1 * (cy v) = (xi x2 cy, x0 cy, x1 cy)
    u32 px[6] = {f.c1.c2.c0, f.c1.c2.c1, f.c1.c0.c0, f.c1.c0.c1, f.c1.c1.c0, f.c1.c1.c1}, py[6], pr[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) py[k] = cy;
    wmuln<6>(pr, px, py, c);
    const F6 t1 = {f2_mul_xi<8>({pr[0], pr[1]}, c), {pr[2], pr[3]}, {pr[4], pr[5]}};  // < 10p, < 2p, < 2p
    return f12_reduce({f6_addn(t0, f6_mul_v<8>(t1, c), c), f6_sub<64>(m, f6_addl(t0, t1), c)}, c);
}
// a^(p^6): the w half negated.  R-form in and out
__device__ __forceinline__ F12 f12_conj(const F12& a, const Ctx& c) {
    const F6 n = {{wneg8(a.c1.c0.c0, c), wneg8(a.c1.c0.c1, c)}, {wneg8(a.c1.c1.c0, c), wneg8(a.c1.c1.c1, c)}, {wneg8(a.c1.c2.c0, c), wneg8(a.c1.c2.c1, c)}};
    return {a.c0, f6_reduce(n, c)};
}
// a^p: every Fp2 coefficient conjugated (c1 <= 8p) and multiplied by g[k] = xi^(k (p-1) / 6) for the coefficient of w^k
// (g[0] = 1 included, so that every coefficient comes out of the same product); frob = the six constants, canonical
__device__ __forceinline__ F12 f12_frobenius(const F12& a, const u32* __restrict__ frob, const Ctx& c) {
    const F2 in[6] = {a.c0.c0, a.c1.c0, a.c0.c1, a.c1.c1, a.c0.c2, a.c1.c2};  // coefficients of w^0 .. w^5
    F2 x[6], y[6], t[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        x[k] = {in[k].c0, wneg8(in[k].c1, c)};
        y[k] = {frob[(2 * k) * 16 + c.li], frob[(2 * k + 1) * 16 + c.li]};
    }
    f2_muln<6>(t, x, y, c);
    return f12_reduce({{t[0], t[2], t[4]}, {t[1], t[3], t[5]}}, c);
}
// 1 / a as host_pairing.h's f12_inv / f6_inv / f2_inv, the one Fp inversion by winv.  R-form in and out (0 for a = 0)
__device__ __forceinline__ F12 f12_inv(const F12& a, const Ctx& c) {
    F6 n;
    {
        F2 x[12], y[12], t[12];
        f6_mul_pre(x, y, a.c0, a.c0, c);
        f6_mul_pre(x + 6, y + 6, a.c1, a.c1, c);
        f2_muln<12>(t, x, y, c);
        const F6 s0 = f6_mul_post(t, c), s1 = f6_mul_post(t + 6, c);  // < 116p
        n = f6_reduce(f6_sub<512>(s0, f6_mul_v<128>(s1, c), c), c);   // subtrahend < 244p
    }
    F6 abc;
    {
        const F2 x[6] = {n.c0, n.c1, n.c2, n.c0, n.c1, n.c0}, y[6] = {n.c0, n.c2, n.c2, n.c1, n.c1, n.c2};
        F2 t[6];
        f2_muln<6>(t, x, y, c);  // n0^2, n1 n2, n2^2, n0 n1, n1^2, n0 n2, each < 10p
        abc = f6_reduce({f2_sub<64>(t[0], f2_mul_xi<32>(t[1], c), c), f2_sub<32>(f2_mul_xi<32>(t[2], c), t[3], c), f2_sub<32>(t[4], t[5], c)}, c);
    }
    F2 fi;
    {
        const F2 x[3] = {n.c0, n.c2, n.c1}, y[3] = {abc.c0, abc.c1, abc.c2};
        F2 t[3];
        f2_muln<3>(t, x, y, c);
        const F2 s = f2_addn(t[0], f2_mul_xi<32>(f2_addn(t[1], t[2], c), c), c);  // < 62p
        u32 fv[2] = {s.c0, s.c1}, sq[2];
        wreduce<2>(fv, c);
        wmuln<2>(sq, fv, fv, c);
        const u32 ni = winv(waddn(sq[0], sq[1], c), c);
        const u32 nn[2] = {ni, ni};
        wmuln<2>(sq, fv, nn, c);
        fi = {sq[0], wneg8(sq[1], c)};  // c1 <= 8p
    }
    F6 d;
    {
        const F2 x[3] = {abc.c0, abc.c1, abc.c2}, y[3] = {fi, fi, fi};
        F2 t[3];
        f2_muln<3>(t, x, y, c);
        d = f6_reduce({t[0], t[1], t[2]}, c);
    }
    F2 x[12], y[12], t[12];
    f6_mul_pre(x, y, a.c0, d, c);
    f6_mul_pre(x + 6, y + 6, a.c1, d, c);
    f2_muln<12>(t, x, y, c);
    const F6 r0 = f6_mul_post(t, c), r1 = f6_mul_post(t + 6, c);
    F6 z;  // zero, to negate r1 < 116p under 128p
    z.c0 = z.c1 = z.c2 = {0u, 0u};
    return f12_reduce({r0, f6_sub<128>(z, r1, c)}, c);
}
__device__ __forceinline__ F12 f12_one(const Ctx& c) {
    F12 r;
    r.c0.c0 = {c.one, 0u};
    r.c0.c1 = r.c0.c2 = r.c1.c0 = r.c1.c1 = r.c1.c2 = {0u, 0u};
    return r;
}
// a == 1 exactly, a R-form; xs = 16 words of exchange scratch of the wave
__device__ __forceinline__ bool f12_is_one(const F12& a, const Ctx& c, u32* xs) {
    u32 v[12];
    f12_to_arr(v, a);
    bool ok = g1w::is_zero_mod_p(wsubk<8>(v[0], c.one, c), xs, c.lane);
#pragma unroll 1
    for (int k = 1; k < 12; ++k) {
        u32 w = v[1];
#pragma unroll
        for (int q = 2; q < 12; ++q) w = k == q ? v[q] : w;
        ok = g1w::is_zero_mod_p(w, xs, c.lane) && ok;
    }
    return ok;
}

// ---------------------------------------------------------------- the two pairs of a check
// sh + NSLOTS * SLOT_WORDS: per pair Z^3, X*Z, Y (16 words each); a pair is skipped when its G1 side has Z = 0 mod p
// or its table is the table of infinity.
struct Pairs {
    const u32* tab[2];  // device line tables (TABLE_WORDS each), nullptr = infinity
    bool skip[2];
};
__device__ __forceinline__ u32* pair_words(u32* sh, int k) { return sh + NSLOTS * SLOT_WORDS + k * PAIR_WORDS; }
__device__ __forceinline__ u32* xchg_words(u32* sh) { return sh + NSLOTS * SLOT_WORDS + 2 * PAIR_WORDS; }

// limb li of a blst coordinate (12 saturated words, any 384-bit value): bit re-slicing as fp28::unpack
__device__ __forceinline__ u32 unpack_limb(const u32* __restrict__ w12, int li) {
    if (li >= fp28::L) return 0u;
    const int bit = 28 * li, w = bit >> 5, s = bit & 31;
    const u64 two = (u64)w12[w] | (w + 1 < 12 ? (u64)w12[w + 1] << 32 : 0);
    return (u32)(two >> s) & fpw::MASK;
}
// The G1 sides of e(a1, A2) == e(b1, B2) as the product e(-a1, A2) e(b1, B2): Jacobian X, Y, Z in blst's Montgomery form.
// The host divides by Z; here the line is scaled by Z^3 instead — c Z^3 + (-lambda X Z) v + Y (v w) — a factor of Fp the
// final exponentiation kills, so the verdict is the one of (X / Z^2, Y / Z^3) for every Z != 0 mod p.  A side is skipped
// for Z = 0 mod p; the host tests for all-zero words, the same thing for canonical coordinates (below p), which is what
// the entry point asks for.
__device__ __forceinline__ void pairs_prepare(Pairs& pr, u32* sh, const u32* __restrict__ a1, const u32* __restrict__ b1, const Ctx& c) {
    constexpr u32 FB[16] = {fp28::from_blst_l(0), fp28::from_blst_l(1), fp28::from_blst_l(2),  fp28::from_blst_l(3),
                            fp28::from_blst_l(4), fp28::from_blst_l(5), fp28::from_blst_l(6),  fp28::from_blst_l(7),
                            fp28::from_blst_l(8), fp28::from_blst_l(9), fp28::from_blst_l(10), fp28::from_blst_l(11),
                            fp28::from_blst_l(12), fp28::from_blst_l(13), 0u, 0u};
    u32 in[6], fb[6], m[6];  // X, Y, Z of a1, of b1: values < 2^384 < 10p, limbs < 2^28
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        in[k] = unpack_limb(a1 + 12 * k, c.li);
        in[3 + k] = unpack_limb(b1 + 12 * k, c.li);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) fb[k] = FB[c.li];
    wmuln<6>(m, in, fb, c);  // R-form, radix 2^392
    u32* xs = xchg_words(sh);
    pr.skip[0] = pr.tab[0] == nullptr || g1w::is_zero_mod_p(m[2], xs, c.lane);
    pr.skip[1] = pr.tab[1] == nullptr || g1w::is_zero_mod_p(m[5], xs, c.lane);
    const u32 x1[4] = {m[2], m[0], m[5], m[3]}, y1[4] = {m[2], m[2], m[5], m[5]};
    u32 t[4];
    wmuln<4>(t, x1, y1, c);  // Z^2, X Z of a1; of b1
    const u32 x2[2] = {t[0], t[2]}, y2[2] = {m[2], m[5]};
    u32 z3[2];
    wmuln<2>(z3, x2, y2, c);
    fpw::wave_sync();
    if (c.row == 0) {
        u32* p0 = pair_words(sh, 0);
        u32* p1 = pair_words(sh, 1);
        p0[c.li] = z3[0], p0[16 + c.li] = t[1], p0[32 + c.li] = wneg8(m[1], c);  // -a1: Y negated, <= 8p
        p1[c.li] = z3[1], p1[16 + c.li] = t[3], p1[32 + c.li] = m[4];
    }
    fpw::wave_sync();
}

// f * line_k(step) for both pairs: per pair one step of four Fp products (c Z^3, lambda X Z) and one sparse product
__device__ __forceinline__ F12 line_step(F12 f, const Pairs& pr, const u32* sh, u32 step, const Ctx& c) {
#pragma unroll 1
    for (int k = 0; k < 2; ++k) {
        if (k ? pr.skip[1] : pr.skip[0]) continue;
        const u32* e = (k ? pr.tab[1] : pr.tab[0]) + (size_t)step * LINE_WORDS + c.li;
        const u32* pw = sh + NSLOTS * SLOT_WORDS + k * PAIR_WORDS + c.li;
        const u32 z3 = pw[0], xz = pw[16], y = pw[32];
        const u32 x[4] = {e[32], e[48], e[0], e[16]}, yv[4] = {z3, z3, xz, xz};
        u32 t[4];
        wmuln<4>(t, x, yv, c);
        f = f12_mul_line(f, {t[0], t[1]}, {wneg8(t[2], c), wneg8(t[3], c)}, y, c);
    }
    return f;
}

// The interpreter: every operation loads its operands from the slots of the wave, and stores an R-form result.  DUMP (the
// device harness of the tests): the twelve result registers of every lane also go to dump[12][64], the last operation's
// staying there.
template <bool DUMP = false>
__device__ __forceinline__ void run_program(const u32* __restrict__ prog, int nprog, u32* sh, const Pairs& pr,
                                            const u32* __restrict__ frob, const Ctx& c, u32* dump = nullptr) {
#pragma unroll 1
    for (int pc = 0; pc < nprog; ++pc) {
        const u32 w = (u32)__builtin_amdgcn_readfirstlane((int)prog[pc]);
        const u32 op = w & 255u, d = (w >> 8) & 255u, a = (w >> 16) & 255u, b = w >> 24;
        if (op == OP_END) break;
        fpw::wave_sync();  // the store of the previous operation
        F12 r;
        if (op == OP_ONE) r = f12_one(c);
        else if (op == OP_MUL) r = f12_mul(f12_load(sh, a, c), f12_load(sh, b, c), c);
        else if (op == OP_SQR) r = f12_sqr(f12_load(sh, a, c), c);
        else if (op == OP_CSQR) r = f12_cyclotomic_sqr(f12_load(sh, a, c), c);
        else if (op == OP_CONJ) r = f12_conj(f12_load(sh, a, c), c);
        else if (op == OP_FROB) r = f12_frobenius(f12_load(sh, a, c), frob, c);
        else if (op == OP_INV) r = f12_inv(f12_load(sh, a, c), c);
        else r = line_step(f12_load(sh, a, c), pr, sh, b, c);
        fpw::wave_sync();  // every lane has its operands
        f12_store(sh, d, r, c);
        if (DUMP) {
            u32 v[12];
            f12_to_arr(v, r);
#pragma unroll
            for (int k = 0; k < 12; ++k) dump[64 * k + c.lane] = v[k];
        }
    }
    fpw::wave_sync();
}

}  // namespace fp12w
