// The addition chain of k_fbw_accum over fp30s::Fe (13 signed limbs of 30 bits, Montgomery radix 2^390): g1::chain_add
// (g1_28.hip.h) with 338 multiply-adds per product instead of 392.  Partial sums and every other kernel keep fp28; the
// wide table holds the same integers as it did in fp28 form, sliced into this form's limbs (WidePt30 below).
//
// The radix mismatch costs no multiplication.  A table coordinate is stored as x * 2^392 mod p; read in the 2^390
// domain the same integer is 4x.  The pair (4x, 8y) is the image of (x, y) under (x, y) -> (u^2 x, u^3 y), u = 2, an
// isomorphism of y^2 = x^3 + 4 onto E': y^2 = x^3 + 256, and the a = 0 chord and tangent formulas never use b.  So a
// lane takes the stored x and y as they are (the table's slot, g1s::WidePt30, holds them re-sliced: fp30s::from28, bits
// only, done once when the table is written), takes y twice where R is formed (a shift inside that subtraction), and
// adds on E'.  to_xyzz28 maps its one partial sum back: with lambda = 2 the class
// (l^2 X, l^3 Y, l^2 ZZ, l^3 ZZZ) of the preimage has the Montgomery-2^392 integers 4 X', 4 Y', 16 ZZ', 32 ZZZ' of the
// 2^390 integers X', Y', ZZ', ZZZ' held here: four products by constants, no inversion.
//
// What the accumulator holds, by state (g1::CHAIN_*; intervals in multiples of p, from tests/fp30s_model.py):
//   CHAIN_EMPTY   all-zero limbs
//   CHAIN_AFFINE  x: the table's x re-sliced (limbs 0..11 in [0, 2^30), value in [0, 1)); y: +-2 y_table centred,
//                 (-2, 2); zz = zzz = fp30s::one()
//   CHAIN_XYZZ    x: A - Q of two centred values, limbs 0..11 in (-2^30, 2^30), value in (-2.2, 2.2) — a legal FIRST
//                 operand of fp30s::mul, and it only ever is one (Q = X1 * PP) or goes through a carry pass (P);
//                 y, zz, zzz: products, centred, (-0.55, 0.55)  (the model reaches 2.03 and 0.52)
// The steps of an addition onto a sum, with the carry passes where the operand rule of fp30s.hip.h asks for them:
//   U2 = x2 * ZZ1, S2 = y2 * ZZZ1           x2, y2 unsigned limbs against centred ones (30.3 * 2^58 per column)
//   P = U2 - X1, R = +-2 S2 - Y1             lazy, limbs <= 2^29 + 2^30: the zero tests read these (limb 0 is the
//                                            value mod 2^30 in any form); then their carry passes, behind the branch
//   PP = P^2, PPP = P * PP, Q = X1 * PP, RR = R^2
//   A = carry(RR - PPP - Q)                  limbs <= 3 * 2^29
//   X3 = A - Q  (lazy, see CHAIN_XYZZ)       R^2 - 2Q - PPP limb-wise would reach 2^31 - 1 before its carry is added
//   V = carry(2Q - A) = Q - X3               limbs <= 3 * 2^29
//   Y3 = R * V + (-Y1) * PPP                 fp30s::mul2, four centred operands
//   ZZ3 = ZZ1 * PP, ZZZ3 = ZZZ1 * PPP
// Exceptional cases, states and the order of the stores on every path are those of g1::chain_add.
#pragma once
#include <cstddef>
#include "fp30s.hip.h"
#include "g1_28.hip.h"

namespace g1s {
using fp30s::Fe;
using fp30s::Seeds;
using g1::CHAIN_AFFINE;
using g1::CHAIN_EMPTY;
using g1::CHAIN_XYZZ;

struct Xyzz {
    Fe x, y, zzz, zz;
};

// Slot of the wide fixed-base table (msm.hip: k_fbw_affine writes it, k_fbw_accum and k_fbw_accum_quad read it).
// x and y are fp30s::from28 of the canonical fp28 value: the SAME integers x * 2^392 mod p and y * 2^392 mod p that
// g1::WidePt held, in the "unsigned" limb form of fp30s.hip.h (limbs 0..11 in [0, 2^30), the rest in the top limb) —
// not centred, y not doubled, not moved to E'.  The chain of k_fbw_accum takes them as they are (the re-slicing was 78
// instructions of every mixed addition); a reader that computes in fp28 (k_fbw_accum_quad) converts back with
// fp30s::to28_unsigned (fp30s::to28 without its carry pass, which is zero throughout on unsigned limbs: on that
// kernel's latency path the pass was 4 us of a 150 us single-commitment call).
// flags bit0 = multiple of a base at infinity (x = y = 0 then); it stands directly behind y, so that a lane loads
// words 0..26, seven 16-byte loads of the 128-byte line.  The padding is written as zero.
// 128 bytes, cache-line aligned, for the reasons g1::WidePt gives.
struct alignas(128) WidePt30 {
    Fe x, y;
    ff::u32 flags, pad[5];
};
static_assert(sizeof(WidePt30) == 128 && offsetof(WidePt30, flags) == 26 * 4, "WidePt30 slot");

// For a kernel that has just loaded a slot: an empty statement per limb that makes the compiler take the 26 limbs as
// values of their own from here on (no instruction).  Measured, not explained: without it this compiler gives
// k_fbw_accum 302 registers instead of 236 (256 and 46 accumulation registers used as spill space: one wave per
// SIMD instead of two, and copies to and from them around the loop over a lane's scalars).  Nothing on the host.
FF_HD void hold(WidePt30& s) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < fp30s::L; ++i) {
        asm("" : "+v"(s.x.v[i]));
        asm("" : "+v"(s.y.v[i]));
    }
#else
    (void)s;
#endif
}

FF_HD WidePt30 pack_slot(const fp28::Fe& x, const fp28::Fe& y, ff::u32 flags) {  // x, y canonical
    WidePt30 o;
    o.x = fp30s::from28(x);
    o.y = fp30s::from28(y);
    o.flags = flags;
#pragma unroll
    for (int i = 0; i < 5; ++i) o.pad[i] = 0;
    return o;
}

FF_HD void set_inf(Xyzz& p) {
    p.x = fp30s::zero();
    p.y = fp30s::zero();
    p.zz = fp30s::zero();
    p.zzz = fp30s::zero();
}

// 2 * (x2, y2) on E' (mdbl-2008-s-1); x2 centred, y2 = +-2 y_table centred.  Off the hot path: a carry pass wherever a
// sum is formed.
FF_HD void dbl_affine(Xyzz& out, const Fe& x2, const Fe& y2, const Seeds& sd) {
    using namespace fp30s;
    const Fe u = carry(add(y2, y2));
    const Fe zz = sqr(u, sd);
    const Fe zzz = mul(zz, u, sd);
    const Fe s = mul(x2, zz, sd);
    const Fe m = sqr(x2, sd);
    const Fe m3 = carry(add(add(m, m), m));
    const Fe x3 = carry(sub(sqr(m3, sd), add(s, s)));
    const Fe y3 = mul2(m3, carry(sub(s, x3)), neg(zzz), y2, sd);
    out.x = x3;
    out.y = y3;
    out.zz = zz;
    out.zzz = zzz;
}

// P = 0 (mod p): equal points -> the tangent, opposite points -> empty.  True if it was one of the two.  p, r: any limbs.
FF_HD bool exceptional(Xyzz& acc, ff::u32& st, const Fe& p, const Fe& r, const Fe& x2, const Fe& y2, ff::u32 m, const Seeds& sd) {
    using namespace fp30s;
    if (!is_zero_mod_p(p)) return false;
    if (is_zero_mod_p(r)) {
        dbl_affine(acc, carry(x2), carry(dbl_signed(carry(y2), m)), sd);
        st = CHAIN_XYZZ;
    } else {
        // (the stores in the order every path ends on: g1::chain_add says why)
        acc.x = zero();
        acc.y = zero();
        acc.zz = zero();
        acc.zzz = zero();
        st = CHAIN_EMPTY;
    }
    return true;
}

// the common part of an addition; SUM: onto a sum (ZZ3 = ZZ1 * PP, ZZZ3 = ZZZ1 * PPP), else onto a single table point
template <bool SUM>
FF_HD void finish(Xyzz& acc, const Fe& p, const Fe& r, const Seeds& sd) {
    using namespace fp30s;
    const Fe pp = sqr(p, sd);
    const Fe ppp = mul(p, pp, sd);
    const Fe q = mul(acc.x, pp, sd);
    const Fe a = carry(sub(sub(sqr(r, sd), ppp), q));
    const Fe v = carry(sub(add(q, q), a));
    const Fe y3 = mul2(r, v, neg(acc.y), ppp, sd);
    acc.x = sub(a, q);
    acc.y = y3;
    acc.zz = SUM ? mul(acc.zz, pp, sd) : pp;
    acc.zzz = SUM ? mul(acc.zzz, ppp, sd) : ppp;
}

// acc += (x, y) for m = 0, acc -= (x, y) for m = 0xffffffff; (x2, y2) a slot of the wide table (WidePt30: unsigned
// limbs of the canonical value, not infinity).  sd: fp30s::seeds(), made at the top of the kernel.
// The addition onto a sum and the one onto a single point are two copies of the code, not one with `if (sum)` around
// the four products by ZZ1 and ZZZ1 as in g1::chain_add.  A signed 32 x 32 -> 64 product is one multiply-add to this
// compiler only while it sees, in the block of the product, that both operands were widened from 32 bits; where two
// paths join, it widens an operand they share once per path and joins the WIDE values, and every product of that
// operand behind the join becomes an unsigned multiply-add and three fix-up instructions (measured: 598 v_mul_lo_u32
// in the addition instead of 91).  Unsigned products (fp28) do not have the problem.
FF_HD void chain_add(Xyzz& acc, ff::u32& st, const Fe& x2, const Fe& y2, ff::u32 m, const Seeds& sd) {
    using namespace fp30s;
    // (the zero tests read the LAZY differences — limb 0 is the value mod 2^30 in any form — and the carry passes stand
    // behind the branch, in the block of the products that take P and R: see above)
    if (st == CHAIN_XYZZ) {
        const Fe dp = sub(mul(x2, acc.zz, sd), acc.x);
        const Fe dr = sub(dbl_signed(mul(y2, acc.zzz, sd), m), acc.y);
        if (exceptional(acc, st, dp, dr, x2, y2, m, sd)) return;
        finish<true>(acc, carry(dp), carry(dr), sd);
    } else if (st == CHAIN_AFFINE) {
        const Fe dp = sub(x2, acc.x);
        const Fe dr = sub(dbl_signed(carry(y2), m), acc.y);
        if (exceptional(acc, st, dp, dr, x2, y2, m, sd)) return;
        finish<false>(acc, carry(dp), carry(dr), sd);
        st = CHAIN_XYZZ;
    } else {
        acc.x = x2;
        acc.y = carry(dbl_signed(carry(y2), m));
        acc.zz = one();
        acc.zzz = one();
        st = CHAIN_AFFINE;
    }
}

// the same for a point in the fp28 form (canonical limbs): re-sliced here
FF_HD void chain_add(Xyzz& acc, ff::u32& st, const fp28::Fe& x28, const fp28::Fe& y28, ff::u32 m, const Seeds& sd) {
    chain_add(acc, st, fp30s::from28(x28), fp30s::from28(y28), m, sd);
}

// The partial sum back on y^2 = x^3 + 4 in the fp28 form, inside the bounds k_blocksum and g1::dadd expect of a stored
// sum: every coordinate a product by a constant, in (-0.51p, 0.51p), plus p: (0.49p, 1.51p), normalized.
FF_HD void to_xyzz28(g1::Xyzz& out, const Xyzz& acc, ff::u32 st, const Seeds& sd) {
    using namespace fp30s;
    if (st == CHAIN_EMPTY) {  // (the stores in the order of the other path, as in chain_add)
        out.x = fp28::zero();
        out.y = fp28::zero();
        out.zz = fp28::zero();
        out.zzz = fp28::zero();
        return;
    }
    constexpr i32 k4[L] = {0x347fcb8,   -0x18a00000, 0x12002b12, -0x7fcc865, 0x90c7213,  0x1a7e0e88, -0x8c1fc8a,
                           -0x192f497c, 0x17bb09b1,  0x17663c4a, 0x12ca7c51, 0x167f3e80, 0x577a6};  // 4 * 2^390 mod p
    constexpr i32 k16[L] = {0xd204835,  -0xa7c0000,  -0xd3f53b5, -0xaf3213f,  -0xcc45bd3, -0x195249ba, 0xbcc1767,
                            0x8619d2e,  -0xdeb3db5,  -0x1401c05, -0x1e7ac075, 0x1f6e9a08, -0x42279};  // 16 * 2^390
    constexpr i32 k32[L] = {0x1a40906a, -0x14f80000, -0x1a7ea76a, -0x15e6427e, -0x1988b7a6, 0xd5b6c8c, 0x17982ecd,
                            0x10c33a5c, -0x1bd67b6a, -0x280380a,  0x30a7f16,   -0x122cbf1,  -0x844f1};  // 32 * 2^390
    const Fe c4 = constant(k4), pf = p_fe();
    out.x = to28(add(mul(acc.x, c4, sd), pf));
    out.y = to28(add(mul(acc.y, c4, sd), pf));
    out.zz = to28(add(mul(acc.zz, constant(k16), sd), pf));
    out.zzz = to28(add(mul(acc.zzz, constant(k32), sd), pf));
}

// The same for a lane of the GLV form: part = 0 sums k1 digits and gets what the form above gives; part = 1 sums k2
// digits against the same table entries and owes its sum the endomorphism psi(x, y) = (beta x, -y) = [x^2](x, y).
// psi(X, Y, ZZ, ZZZ) = (beta X, -Y, ZZ, ZZZ) holds on E' with the same beta: the map (x, y) -> (4x, 8y) between the two
// curves commutes with it.  So psi costs no product of its own: X goes back through 4 * beta * 2^390 mod p (the integer
// beta28() holds, beta * 2^392) instead of 4 * 2^390, selected limb by limb without a branch, and Y is negated limb-wise
// before its product by the unchanged constant.  Bounds: the constant for beta is centred like k4, value in
// (-p/2, p/2), so the product's interval is the one of the form above; |-Y| = |Y|, and the negation of a centred value
// has limbs in [-2^29, 2^29], which the operand rule of fp30s::mul admits (tests/test_table_slot30_cpu.py runs both
// through the model).  The stored sum is inside the same interval, (0.49p, 1.51p), normalized.
FF_HD void to_xyzz28(g1::Xyzz& out, const Xyzz& acc, ff::u32 st, ff::u32 part, const Seeds& sd) {
    using namespace fp30s;
    if (st == CHAIN_EMPTY) {  // (the stores in the order of the other path, as in chain_add)
        out.x = fp28::zero();
        out.y = fp28::zero();
        out.zz = fp28::zero();
        out.zzz = fp28::zero();
        return;
    }
    constexpr i32 k4[L] = {0x347fcb8,   -0x18a00000, 0x12002b12, -0x7fcc865, 0x90c7213,  0x1a7e0e88, -0x8c1fc8a,
                           -0x192f497c, 0x17bb09b1,  0x17663c4a, 0x12ca7c51, 0x167f3e80, 0x577a6};  // 4 * 2^390 mod p
    constexpr i32 k4b[L] = {0xa75929a,   -0xa5f921a, -0xdd5c16,   0x116af00b, -0x181b1a45, 0x45d579c, 0xf1b4814,
                            0xe1f5b41,   -0x134f351d, 0x131d2d53, -0x1ec74af6, 0x19381996, 0x76f2b};  // 4 beta 2^390
    constexpr i32 k16[L] = {0xd204835,  -0xa7c0000,  -0xd3f53b5, -0xaf3213f,  -0xcc45bd3, -0x195249ba, 0xbcc1767,
                            0x8619d2e,  -0xdeb3db5,  -0x1401c05, -0x1e7ac075, 0x1f6e9a08, -0x42279};  // 16 * 2^390
    constexpr i32 k32[L] = {0x1a40906a, -0x14f80000, -0x1a7ea76a, -0x15e6427e, -0x1988b7a6, 0xd5b6c8c, 0x17982ecd,
                            0x10c33a5c, -0x1bd67b6a, -0x280380a,  0x30a7f16,   -0x122cbf1,  -0x844f1};  // 32 * 2^390
    const ff::u32 m = 0u - (part & 1u);
    Fe cx, y;
#pragma unroll
    for (int i = 0; i < L; ++i) {
        cx.v[i] = m ? k4b[i] : k4[i];
        y.v[i] = (i32)(((ff::u32)acc.y.v[i] ^ m) - m);
    }
    const Fe pf = p_fe();
    out.x = to28(add(mul(acc.x, cx, sd), pf));
    out.y = to28(add(mul(y, constant(k4), sd), pf));
    out.zz = to28(add(mul(acc.zz, constant(k16), sd), pf));
    out.zzz = to28(add(mul(acc.zzz, constant(k32), sd), pf));
}

}  // namespace g1s
