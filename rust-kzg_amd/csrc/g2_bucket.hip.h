// The per-lane parts of the bucket engines over signed base-256 digits, host- and device-compilable so that
// tests/test_g2_msm_cpu.py runs on the host what the kernels of g2msm.hip run: the recoding of a scalar (groupmul.hip
// walks a table of one base with it, g2msm.hip sorts its digits into buckets), the entries a scalar yields, the cutting
// of a bucket into segments level by level, the chain of a segment, and the weighting of a bucket sum by its index.
// Only routines of g2_28.hip.h, inside the bounds its table states:
//   a chain over table entries    acc is infinity, the entry itself (canonical, Z = one) or what madd left (X, Y < 3,
//                                 Z < 10) or dbl (X, Y < 2, Z < 10): each an input of madd_tab
//   a chain over partial sums     operands are chain results (X, Y < 3, Z < 10) or sums of g2::add (X, Y < 2, Z < 10):
//                                 g2::add takes X, Y < 3, Z < 10 on both sides
//   weigh                         dbl takes X, Y < 15, Z < 21; its output and that of add go into add
// Every addition is a complete one: equal operands, opposite operands and an operand at infinity are all right.
#pragma once
#include "ff.hip.h"
#include "g2_28.hip.h"

namespace g2b {
using ff::u32;

constexpr int WBITS = 8;                // window width
constexpr int NWIN = 32;                // windows of a 256-bit scalar
constexpr int HALF = 1 << (WBITS - 1);  // the largest digit, and the buckets of a batch item: 1 .. 128
constexpr u32 NEG_BIT = 0x80000000u;    // of an entry: the table point is subtracted

// digit w of the signed base-256 recoding of the plain (non-Montgomery) scalar k: returns |d_w| in [0, 128] and sets
// neg to all-ones when d_w < 0; carry in and out.  A digit above 128 becomes d - 256 and carries one into the next
// window; the top window of a scalar below r < 0x74 * 2^248 holds at most 0x73 + 1, so nothing carries out.
FF_HD u32 signed_digit(const ff::Fr& k, int w, u32& carry, u32& neg) {
    const u32 v = ((k.v[w >> 2] >> (8 * (w & 3))) & 0xffu) + carry;
    carry = v > (u32)HALF ? 1u : 0u;
    neg = 0u - carry;
    return carry ? 256u - v : v;
}

// The entries of scalar k (plain form) at point i of a table of npoints points per window: one per non-zero digit whose
// table point T[w * npoints + i] is not infinite (bit w of inf_mask says it is).  f(bucket, value) is called for each:
// bucket in 1 .. 128 is |d_w|, value the table index with NEG_BIT for a negative digit.
template <class F>
FF_HD void for_each_entry(const ff::Fr& k, u32 i, u32 npoints, u32 inf_mask, F&& f) {
    u32 carry = 0;
#pragma unroll 1
    for (int w = 0; w < NWIN; ++w) {
        u32 neg;
        const u32 d = signed_digit(k, w, carry, neg);
        if (d == 0 || ((inf_mask >> w) & 1)) continue;
        f(d, ((u32)w * npoints + i) | (neg & NEG_BIT));
    }
}

// the key of item s in a run of K keys whose items start at off[0 .. K] (off[0] == 0, s < off[K]): the one key with
// off[key] <= s < off[key + 1], whatever empty keys lie around it
FF_HD u32 key_of(const u32* off, u32 K, u32 s) {
    u32 lo = 0, hi = K;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (off[mid] <= s) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A run of c items is cut into segments of `seg` items, the last one shorter: ceil(c / seg) of them, none for c == 0.
FF_HD u32 segments(u32 c, u32 seg) { return (c + seg - 1) / seg; }
// items [lo, hi) of segment j < segments(c, seg)
FF_HD void segment_range(u32 c, u32 seg, u32 j, u32& lo, u32& hi) {
    lo = j * seg;
    hi = c - lo < seg ? c : lo + seg;
}

// acc = the sum of the table points the entries e[0 .. n) name, signs applied
FF_HD void chain_entries(g2::Jac& acc, const g2::AffPt* tab, const u32* e, u32 n) {
    g2::set_inf(acc);
#pragma unroll 1
    for (u32 t = 0; t < n; ++t) g2::madd_tab(acc, tab[e[t] & ~NEG_BIT], e[t] & NEG_BIT);
}
// acc = the sum of the partial sums p[0 .. n)
FF_HD void chain_partials(g2::Jac& acc, const g2::Jac* p, u32 n) {
    g2::set_inf(acc);
#pragma unroll 1
    for (u32 t = 0; t < n; ++t) g2::add(acc, p[t]);
}

// out = w * b for a bucket index w in 1 .. 128: left to right over its 8 bits, 7 doublings and at most 7 additions
FF_HD void weigh(g2::Jac& out, const g2::Jac& b, u32 w) {
    g2::set_inf(out);
    if (g2::is_inf(b)) return;
#pragma unroll 1
    for (int bit = WBITS - 1; bit >= 0; --bit) {
        if (!g2::is_inf(out)) g2::dbl(out);
        if ((w >> bit) & 1) g2::add(out, b);
    }
}

// p = 2^8 p: the step from one window of a point's table column to the next
FF_HD void next_window(g2::Jac& p) {
    if (g2::is_inf(p)) return;
#pragma unroll 1
    for (int i = 0; i < WBITS; ++i) g2::dbl(p);
}

}  // namespace g2b
