// Fp for the addition chain of k_fbw_accum: 13 SIGNED limbs of 30 bits, Montgomery radix 2^390.
//
// Why a second unsaturated form beside fp28 (14 x 28 bits): a product and its reduction are 2 * 13^2 = 338 multiply-adds
// instead of 2 * 14^2 = 392, and the kernel is bound by the issue of exactly those (profiles/NOTES.md, sections 26, 34).
// 26 unsigned products of 60 bits do not fit a 64-bit column; 26 signed ones of 58 bits do.
//
// Representation: value = sum v[i] * 2^(30 i), every limb an int32; values may be negative and are tracked as
// intervals of multiples of p (tests/fp30s_model.py propagates them and the column bounds quoted below).
//   "centred"   limbs 0..11 in [-2^29, 2^29], the top limb carries the rest of the value with its sign
//   "unsigned"  limbs 0..11 in [0, 2^30), top limb >= 0 (a re-sliced table coordinate, from28)
//
// Operand rule:
//   mul(a, b)    a centred or unsigned, b centred; |top limbs| < 2^26.  A column is at most 12 full products of
//                2^30 * 2^29, two with a top limb, and the quotient digits against p (sum |p_j| * 2^29 < 6.21 * 2^58):
//                30.3 * 2^58 + a carry < 2^63 (model: 2^62.92).  Both centred: 18.3 * 2^58.
//   sqr(a)       a centred: 18.3 * 2^58
//   mul2         a*b + c*d on ONE chain, all four centred, |top limbs| < 2^26: 24 full products, 30.3 * 2^58 < 2^63.
//                Without the bound on the top limbs a column would reach 39 * 2^58 > 2^63: the callers' values are
//                below 64p in absolute value, which is what the bound needs.
//   result       centred, limbs 0..11 in [-2^29, 2^29), congruent to the product * 2^-390, and
//                |value| < p / 2 * (1 + 2^-28) + |product| / 2^390  (p / 2^390 < 2^-9.3: 0.51p for |product| <= 4 p^2)
//   add/sub/neg  limb-wise, no pads; a lazy sum of two centred values needs carry() before it is a multiplicand
// Column sums are kept in unsigned 64-bit arithmetic (wrapping, no undefined behaviour); the bounds above say that the
// true signed value fits, so the arithmetic shift that ends a column sees the true value.
#pragma once
#include "fp28.hip.h"

namespace fp30s {
using ff::u32;
using ff::u64;
typedef int32_t i32;
typedef int64_t i64;

constexpr int L = 13;
constexpr u32 MASK = (1u << 30) - 1;
constexpr u32 HALF = 1u << 29;
constexpr u32 PINV = 0x00030003u;  // p^-1 mod 2^32

struct Fe {
    i32 v[L];
};

FF_HD constexpr i32 pl(int i) {  // p, centred
    constexpr i32 t[L] = {-0x5555,     -0x18040000, 0x153ffffc,  -0x15000054, -0xf09dbe1, 0x34a83db, 0x112bf673,
                          0x12e13ce1,  -0x13289b89, 0x1ed90d2f,  -0x165b4e46, -0x571a006, 0x1a0112};
    return t[i];
}

FF_HD i32 sext30(u32 x) { return (i32)(x << 2) >> 2; }
FF_HD void mad(u64& acc, i32 a, i32 b) { acc += (u64)((i64)a * (i64)b); }
FF_HD void shr30(u64& acc) { acc = (u64)((i64)acc >> 30); }
// the quotient digit of a lower column: m = acc * p^-1 mod 2^30, centred; acc - m * p_0 is a multiple of 2^30
FF_HD i32 digit(u64& acc) {
    const i32 m = sext30((u32)acc * PINV);
    mad(acc, m, -pl(0));
    shr30(acc);
    return m;
}
// an upper column's output limb: the chain was seeded with 2^29, so the low 30 bits less 2^29 are the centred limb and
// the arithmetic shift is the rounded carry
FF_HD i32 limb(u64& acc) {
    const i32 r = (i32)(((u32)acc & MASK) - HALF);
    shr30(acc);
    return r;
}

FF_HD Fe zero() {
    Fe r;
#pragma unroll
    for (int i = 0; i < L; ++i) r.v[i] = 0;
    return r;
}
FF_HD bool is_zero_limbs(const Fe& a) {
    u32 acc = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) acc |= (u32)a.v[i];
    return acc == 0;
}

// The seeds of the columns.  A column is ONE sum: the compiler orders its terms by where in the kernel they were made,
// earliest first, and folds every product into a multiply-add whose addend is the sum so far.  A term that is not a
// product costs a 64-bit addition wherever it stands but in front, so each column gets exactly one such term in front,
// its seed: 2^30 in column 0, which arrives in column 1 as a carry of 1 and is taken back by a seed of 2^30 - 1 there,
// and so on up the lower columns (a multiple of 2^30 does not change a quotient digit); column 13 gets 2^29 - 1 and the
// columns above it 2^29, the rounding bias of limb().  (A sum that starts from two products starts from a bare signed
// 64-bit product, which this compiler expands into an unsigned multiply-add and four fix-up instructions.)  For the
// seeds to come first they have to be made before the operands: a kernel calls seeds() once at its top, on the device
// a scalar load from constant memory, since a literal would be moved to the END of every sum.
struct Seeds {
    u64 first, lower, mid, upper;
};
#if defined(__HIP_DEVICE_COMPILE__)
static __constant__ u32 bias_word = HALF;
FF_HD u32 half() { return bias_word; }
#else
FF_HD u32 half() { return HALF; }
#endif
FF_HD Seeds seeds() {
    const u64 h = half();
    return Seeds{h << 1, (h << 1) - 1, h - 1, h};
}
FF_HD u64 seed(int k, const Seeds& sd) { return k == 0 ? sd.first : k < L ? sd.lower : k == L ? sd.mid : sd.upper; }

// a*b*2^-390 mod p.  Product scanning; the quotient digits' products are SUBTRACTED (-p_j as the constant).  Each
// column in two chains: the carried one takes the digits' products (a constant operand each), the fresh one the
// operands' products.
FF_HD Fe mul(const Fe& a, const Fe& b, const Seeds& sd) {
    i32 m[L];
    Fe r;
    u64 acc = 0;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        u64 f = seed(k, sd);
#pragma unroll
        for (int i = 0; i <= k; ++i) mad(f, a.v[i], b.v[k - i]);
#pragma unroll
        for (int i = 0; i < k; ++i) mad(acc, m[i], -pl(k - i));
        acc += f;
        m[k] = digit(acc);
    }
#pragma unroll
    for (int k = L; k < 2 * L - 1; ++k) {
        u64 f = seed(k, sd);
#pragma unroll
        for (int i = k - L + 1; i < L; ++i) mad(f, a.v[i], b.v[k - i]);
#pragma unroll
        for (int i = k - L + 1; i < L; ++i) mad(acc, m[i], -pl(k - i));
        acc += f;
        r.v[k - L] = limb(acc);
    }
    r.v[L - 1] = (i32)acc;
    return r;
}

// a^2: the off-diagonal products once against 2a (|2 a_i| <= 2^30 fits the signed multiplier)
FF_HD Fe sqr(const Fe& a, const Seeds& sd) {
    i32 m[L], a2[L];
    Fe r;
#pragma unroll
    for (int i = 0; i < L; ++i) a2[i] = (i32)((u32)a.v[i] << 1);
    u64 acc = 0;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        u64 f = seed(k, sd);
#pragma unroll
        for (int i = 0; 2 * i < k; ++i) mad(f, a2[i], a.v[k - i]);
        if ((k & 1) == 0) mad(f, a.v[k / 2], a.v[k / 2]);
#pragma unroll
        for (int i = 0; i < k; ++i) mad(acc, m[i], -pl(k - i));
        acc += f;
        m[k] = digit(acc);
    }
#pragma unroll
    for (int k = L; k < 2 * L - 1; ++k) {
        u64 f = seed(k, sd);
#pragma unroll
        for (int i = k - L + 1; 2 * i < k; ++i) mad(f, a2[i], a.v[k - i]);
        if ((k & 1) == 0) mad(f, a.v[k / 2], a.v[k / 2]);
#pragma unroll
        for (int i = k - L + 1; i < L; ++i) mad(acc, m[i], -pl(k - i));
        acc += f;
        r.v[k - L] = limb(acc);
    }
    r.v[L - 1] = (i32)acc;
    return r;
}

// (a*b + c*d) * 2^-390 mod p under one reduction (see the operand rule for why one column holds both products)
FF_HD Fe mul2(const Fe& a, const Fe& b, const Fe& c, const Fe& d, const Seeds& sd) {
    i32 m[L];
    Fe r;
    u64 acc = 0;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        u64 f = seed(k, sd);
#pragma unroll
        for (int i = 0; i <= k; ++i) mad(f, a.v[i], b.v[k - i]);
#pragma unroll
        for (int i = 0; i <= k; ++i) mad(acc, c.v[i], d.v[k - i]);
#pragma unroll
        for (int i = 0; i < k; ++i) mad(acc, m[i], -pl(k - i));
        acc += f;
        m[k] = digit(acc);
    }
#pragma unroll
    for (int k = L; k < 2 * L - 1; ++k) {
        u64 f = seed(k, sd);
#pragma unroll
        for (int i = k - L + 1; i < L; ++i) mad(f, a.v[i], b.v[k - i]);
#pragma unroll
        for (int i = k - L + 1; i < L; ++i) mad(acc, c.v[i], d.v[k - i]);
#pragma unroll
        for (int i = k - L + 1; i < L; ++i) mad(acc, m[i], -pl(k - i));
        acc += f;
        r.v[k - L] = limb(acc);
    }
    r.v[L - 1] = (i32)acc;
    return r;
}

// ---- linear operations: limb-wise, signed, no pads ----
FF_HD Fe add(const Fe& a, const Fe& b) {
    Fe r;
#pragma unroll
    for (int i = 0; i < L; ++i) r.v[i] = (i32)((u32)a.v[i] + (u32)b.v[i]);
    return r;
}
FF_HD Fe sub(const Fe& a, const Fe& b) {
    Fe r;
#pragma unroll
    for (int i = 0; i < L; ++i) r.v[i] = (i32)((u32)a.v[i] - (u32)b.v[i]);
    return r;
}
FF_HD Fe neg(const Fe& a) {
    Fe r;
#pragma unroll
    for (int i = 0; i < L; ++i) r.v[i] = (i32)(0u - (u32)a.v[i]);
    return r;
}
// 2 * (+-a): m = 0 for +, 0xffffffff for -; |a_i| <= 2^29
FF_HD Fe dbl_signed(const Fe& a, u32 m) {
    Fe r;
#pragma unroll
    for (int i = 0; i < L; ++i) r.v[i] = (i32)((((u32)a.v[i] ^ m) - m) << 1);
    return r;
}

// The carry pass: a lazy value back to centred limbs (limbs 0..11 in [-2^29, 2^29), value unchanged).
// Input limbs 0..11 at most 3 * 2^29 in absolute value (three centred terms, or a doubled one and a plain one): with
// the carry, at most 2 in absolute value, t stays far inside an int32.  The rounded carry is the floor carry plus
// bit 29 of t, so no sum ever has 2^29 added to it: 3 * 2^29 + 2^29 is 2^31, one more than an int32 holds.
FF_HD Fe carry(const Fe& a) {
    Fe r;
    i32 cf = 0, b = 0;
#pragma unroll
    for (int i = 0; i < L - 1; ++i) {
        const i32 t = a.v[i] + cf + b;
        r.v[i] = sext30((u32)t);
        cf = t >> 30;
        b = (t >> 29) & 1;
    }
    r.v[L - 1] = a.v[L - 1] + cf + b;
    return r;
}

FF_HD Fe constant(const i32 (&t)[L]) {
    Fe r;
#pragma unroll
    for (int i = 0; i < L; ++i) r.v[i] = t[i];
    return r;
}
FF_HD Fe one() {  // 2^390 mod p, centred
    constexpr i32 t[L] = {0xd1ff2e,    0x19d80000, -0xb7ff53c,  -0x11ff3219, 0x2431c85,  -0x19607c5e, -0x2307f22,
                          0x9b42da1,   -0x1a113d94, 0x15d98f13, 0x4b29f14,   -0x1a603060, 0x15dea};
    return constant(t);
}
FF_HD Fe p_fe() {
    Fe r;
#pragma unroll
    for (int i = 0; i < L; ++i) r.v[i] = pl(i);
    return r;
}

// exact test a == 0 (mod p) for |value| < 32p, any limbs that are an int32 each.  If a = k p then
// k = a * p^-1 mod 2^30 (centred), and limb 0 holds the value mod 2^30 whatever the other limbs are: a filter of two
// instructions rejects all but 2^-24 of the non-zero values, the exact comparison of a with k p runs only then.
FF_HD bool is_zero_mod_p(const Fe& a) {
    const i32 k = sext30((u32)a.v[0] * PINV);
    // -DKZGAMD_FORCE_EXACT_TESTS: no filter, as in fp28::is_zero_mod_p (for |k| >= 32 the comparison is against a
    // multiple of p the value cannot be)
#if !defined(KZGAMD_FORCE_EXACT_TESTS)
    if ((u32)(k + 32) >= 64u) return false;
#endif
    i64 c = 0;
    u32 diff = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) {
        c += (i64)a.v[i] - (i64)k * pl(i);
        diff |= i < L - 1 ? ((u32)c & MASK) : ((u32)c | (u32)((u64)c >> 32));
        c >>= 30;
    }
    return diff == 0;
}

// ---- conversions: the 14 x 28-bit form of fp28 (the table, the partial sums) ----
// bit re-slicing only: a normalized fp28 value as "unsigned" limbs (0..11 in [0, 2^30), the rest in the top limb)
FF_HD Fe from28(const fp28::Fe& a) {
    Fe r;
#pragma unroll
    for (int i = 0; i < L; ++i) {
        const int bit = 30 * i, j = bit / 28, s = bit - 28 * j;
        u32 w = a.v[j] >> s;
        if (j + 1 < fp28::L) w |= a.v[j + 1] << (28 - s);
        if (j + 2 < fp28::L && 56 - s < 30) w |= a.v[j + 2] << (56 - s);
        r.v[i] = (i32)(i < L - 1 ? (w & MASK) : w);
    }
    return r;
}
// a value in [0, 2^396) with any int32 limbs -> normalized fp28 limbs (a floor carry to digits, then bit re-slicing)
FF_HD fp28::Fe to28(const Fe& a) {
    u32 d[L];
    i32 c = 0;
#pragma unroll
    for (int i = 0; i < L - 1; ++i) {
        const i32 t = a.v[i] + c;
        d[i] = (u32)t & MASK;
        c = t >> 30;
    }
    d[L - 1] = (u32)(a.v[L - 1] + c);
    fp28::Fe r;
#pragma unroll
    for (int j = 0; j < fp28::L; ++j) {
        const int bit = 28 * j, i = bit / 30, s = bit - 30 * i;
        u32 w = d[i] >> s;
        if (i + 1 < L && 30 - s < 28) w |= d[i + 1] << (30 - s);
        r.v[j] = j < fp28::L - 1 ? (w & fp28::MASK) : w;
    }
    return r;
}

// the same for "unsigned" limbs (from28 of a normalized value: a table slot), where the carry pass above has nothing to
// carry: bit re-slicing only, the exact inverse of from28, with no chain of dependent additions in front of it
FF_HD fp28::Fe to28_unsigned(const Fe& a) {
    fp28::Fe r;
#pragma unroll
    for (int j = 0; j < fp28::L; ++j) {
        const int bit = 28 * j, i = bit / 30, s = bit - 30 * i;
        u32 w = (u32)a.v[i] >> s;
        if (i + 1 < L && 30 - s < 28) w |= (u32)a.v[i + 1] << (30 - s);
        r.v[j] = j < fp28::L - 1 ? (w & fp28::MASK) : w;
    }
    return r;
}

}  // namespace fp30s
