// G2 point arithmetic over fp28::Fe, one value per lane: Fp2 = Fp[u]/(u^2 + 1) and points of the twist
// E'(Fp2): y^2 = x^3 + 4(1 + u), in the style of g1_28.hip.h.  host_pairing.h is the specification: f2_mul / f2_sqr
// with the same Karatsuba split, g2_dbl (dbl-2009-l), g2_add (add-2007-bl) with Z2 = 1 and in full, g2_to_affine; every
// routine returns the value the host routine returns (tests/test_g2_lane_cpu.py and tests/test_g2_add_cpu.py compare
// them as canonical residues).  The device build is held to the table below routine by routine, against Python integers,
// by tests/test_g2_arith_gpu.py (tests/device_checks/g2_check.hip, cases in tests/g2_lane_cases.py).
//
// Bounds.  An Fp2 value is two fp28 components, each NORMALIZED (limbs 0..12 < 2^28) with a value below a stated
// multiple of p; "a < K" below means both components of a are normalized with value < K*p.  The rules of fp28.hip.h
// carry over: a product's operands have limbs < 2^30 and a value product < 2^392 * p = 2520 p^2, and it returns a
// normalized value < 2p; sub<K>(a, b) = a + K*p - b needs b < (K - 1).  The Karatsuba sums a0 + a1 are taken lazily
// (limbs < 2^29), so they double the bound of an operand: that is what limits every routine below.
//
//   routine        accepts                                   returns
//   add(a, b)      any a, b with a + b < 2^6                 < a + b
//   dbl(a)         a < 2^5                                   < 2a
//   sub<K>(a, b)   b < K - 1                                 < a + K
//   neg<K>(a)      a < K - 1                                 <= K
//   mul(a, b)      a < A, b < B with A * B <= 630            c0 < 6, c1 < 10     ((a0 + a1)(b0 + b1) < 4AB p^2 <= 2520 p^2)
//   sqr(a)         a < 15                                    c0 < 2, c1 < 4      ((a0 + a1)(a0 + 16p - a1) < 30 * 31 p^2)
//   mul_fe(a, b)   a < A, b < B (an Fe) with A * B <= 2520   < 2
//   red(a)         a < 2^6                                   < 2                 (a multiplication by one per component)
//   is_zero(a)     a < 2^6                                   exact: both components are 0 mod p
// (2^6: what fp28::is_zero_mod_p takes; every sum in this header stays far below it.)
//
//   dbl(P)         X, Y < 15, Z < 21, P not infinity         X, Y < 2, Z < 10
//   madd(P, Q)     X1, Y1 < 3, Z1 < 10 (or P infinity);      X, Y < 3, Z < 10, or one of the states below
//                  Q affine: x, y < 3, not infinity
//   madd_tab(P, e, neg)  P as madd; e a table entry (canonical x, y, or flagged infinite)   as madd; complete
//   add(P, Q)      X, Y < 3, Z < 10 on both sides, or either     X, Y < 2, Z < 10, or infinity; complete
//                  at infinity
// so the output of any of dbl, madd and add is an input of any of them, and a table point (canonical x, y; -Q as
// neg<2>(y) <= 2) an input of madd.  The rare exact-zero tests sit in madd and add alone (H == 0, then r == 0), through
// fp28::is_zero_mod_p, which honours KZGAMD_FORCE_EXACT_TESTS.
#pragma once
#include "fp28.hip.h"
#include "g1_io.hip.h"

namespace g2 {
using ff::u32;
using fp28::Fe;

struct F2 {
    Fe c0, c1;
};

FF_HD F2 zero() { return {fp28::zero(), fp28::zero()}; }
FF_HD F2 one() { return {fp28::one(), fp28::zero()}; }
FF_HD bool is_zero_limbs(const F2& a) { return fp28::is_zero_limbs(a.c0) && fp28::is_zero_limbs(a.c1); }
FF_HD bool is_zero(const F2& a) { return fp28::is_zero_mod_p(a.c0) && fp28::is_zero_mod_p(a.c1); }

FF_HD F2 add(const F2& a, const F2& b) { return {fp28::addn(a.c0, b.c0), fp28::addn(a.c1, b.c1)}; }
FF_HD F2 dbl(const F2& a) { return add(a, a); }
template <int K>
FF_HD F2 sub(const F2& a, const F2& b) {
    return {fp28::sub<K>(a.c0, b.c0), fp28::sub<K>(a.c1, b.c1)};
}
template <int K>
FF_HD F2 neg(const F2& a) {
    return {fp28::neg<K>(a.c0), fp28::neg<K>(a.c1)};
}

// Karatsuba, three products: c0 = a0 b0 - a1 b1, c1 = (a0 + a1)(b0 + b1) - a0 b0 - a1 b1.
// t0, t1, t2 < 2p; c0 = t0 + 4p - t1 < 6p; t0 + t1 < 4p <= 7p, c1 = t2 + 8p - (t0 + t1) < 10p.
// The sums are lazy: limbs < 2^29 against limbs < 2^29, columns <= 14 * 2^58 + 14 * 2^56 < 2^63.
FF_HD F2 mul(const F2& a, const F2& b) {
    const Fe t0 = fp28::mul(a.c0, b.c0), t1 = fp28::mul(a.c1, b.c1);
    const Fe t2 = fp28::mul(fp28::add(a.c0, a.c1), fp28::add(b.c0, b.c1));
    return {fp28::sub<4>(t0, t1), fp28::sub<8>(t2, fp28::addn(t0, t1))};
}
// c0 = (a0 + a1)(a0 - a1), c1 = 2 a0 a1.  a0 + 16p - a1 by sub_lazy<16> (a1 < 15p): limbs < 2^28 + 2^29 against
// limbs < 2^29, columns <= 14 * 1.5 * 2^58 + 14 * 2^56 < 2^63; value < 30p * 31p.
FF_HD F2 sqr(const F2& a) {
    const Fe t = fp28::mul(a.c0, a.c1);
    return {fp28::mul(fp28::add(a.c0, a.c1), fp28::sub_lazy<16>(a.c0, a.c1)), fp28::addn(t, t)};
}
FF_HD F2 mul_fe(const F2& a, const Fe& b) { return {fp28::mul(a.c0, b), fp28::mul(a.c1, b)}; }
// the same value below 2p: a multiplication by one per component (as g1::reduce_xy)
FF_HD F2 red(const F2& a) { return mul_fe(a, fp28::one()); }
// 1 / a = conj(a) / (a0^2 + a1^2) for a < 15, a != 0; returns < 2.  The norm a0^2 + a1^2 < 4p goes through one more
// product so that g1io::inverse gets what it asks for (a product's output).
FF_HD F2 inv(const F2& a) {
    const Fe n = fp28::mul(fp28::addn(fp28::sqr(a.c0), fp28::sqr(a.c1)), fp28::one());
    const Fe ni = g1io::inverse(n);
    return {fp28::mul(a.c0, ni), fp28::mul(fp28::neg<16>(a.c1), ni)};
}

FF_HD F2 from_blst(const ff::Fp in[2]) { return {fp28::from_blst(in[0]), fp28::from_blst(in[1])}; }
FF_HD void to_blst(ff::Fp out[2], const F2& a) {  // a < 2^6 (fp28::to_blst multiplies: < 2520); canonical output
    out[0] = fp28::to_blst(a.c0);
    out[1] = fp28::to_blst(a.c1);
}

// Jacobian point (x = X / Z^2, y = Y / Z^3); infinity <=> Z all-zero limbs, as blst_p2 has Z == 0
struct Jac {
    F2 x, y, z;
};
// table / input point: canonical x, y; flags bit0 = point at infinity
struct alignas(16) AffPt {
    F2 x, y;
    u32 flags, pad[3];
};
static_assert(sizeof(AffPt) == 240, "AffPt slot");

FF_HD void set_inf(Jac& p) { p.x = p.y = p.z = zero(); }
FF_HD bool is_inf(const Jac& p) { return is_zero_limbs(p.z); }
FF_HD void set_affine(Jac& p, const F2& x, const F2& y) {
    p.x = x;
    p.y = y;
    p.z = one();
}

// p = 2p (dbl-2009-l, the value of pairing::g2_dbl: X3 = F - 2D, Y3 = E(D - X3) - 8C, Z3 = 2 Y Z with A = X^2,
// B = Y^2, C = B^2, D = 2((X + B)^2 - A - C) = 4 X B, E = 3A, F = E^2); p not infinity.
//   A, B < 4; 8C = 2 (2B)^2: (2B)^2 < 4, 8C < 8; D = (2X)(2B): 30 * 8 <= 630, D < 10; E < 12; F < 4;
//   F + 32p - 2D < 36 (2D < 20 <= 31), reduced: X3 < 2; D + 4p - X3 < 14; E * that: 12 * 14 <= 630, < 10;
//   that + 16p - 8C < 26, reduced: Y3 < 2; Z3 = (2Y) Z: 30 * 21 = 630, Z3 < 10.
FF_HD void dbl(Jac& p) {
    const F2 A = sqr(p.x), B = sqr(p.y);
    const F2 C8 = dbl(sqr(dbl(B)));
    const F2 D = mul(dbl(p.x), dbl(B));
    const F2 E = add(dbl(A), A);
    const F2 X3 = red(sub<32>(sqr(E), dbl(D)));
    const F2 Y3 = red(sub<16>(mul(E, sub<4>(D, X3)), C8));
    p.z = mul(dbl(p.y), p.z);
    p.x = X3;
    p.y = Y3;
}

// what madd found: MADD_DONE the sum is in p (also when p was infinity: the affine point); MADD_DOUBLE the two are the
// same point, p is untouched and the caller doubles (as g1::dadd_unequal: the doubling stays one site of its own);
// MADD_INF they are opposite points, p is set to infinity.
constexpr u32 MADD_DONE = 0, MADD_DOUBLE = 1, MADD_INF = 2;

// p += (x2, y2), an affine point not at infinity (add-2007-bl with Z2 = 1, the value of pairing::g2_add).
//   Z1Z1 < 4; U2 = x2 Z1Z1: 3 * 4, < 10; S2 = (y2 Z1) Z1Z1: 3 * 10, then 10 * 4, < 10;
//   H = U2 + 4p - X1 < 14, r = S2 + 4p - Y1 < 14 (X1, Y1 < 3); both zero-tested (< 2^6);
//   I = (2H)^2 = 4 H^2 < 16 (H^2 < 4); J = H I: 14 * 16, < 10; V = X1 I: 3 * 16, < 10;
//   (2r)^2 = 4 r^2 < 16; J + 2V < 30 <= 31: X3 = 4r^2 + 32p - J - 2V < 48, reduced: < 2;
//   (2r)(V + 4p - X3): 28 * 14 <= 630, < 10; 2 Y1 J: Y1 J is 3 * 10, < 10, doubled < 20 <= 31: Y3 < 42, reduced: < 2;
//   Z3 = (Z1 + 1)^2 - Z1Z1 - 1 times H = (2 Z1) H: 20 * 14, < 10.
FF_HD u32 madd(Jac& p, const F2& x2, const F2& y2) {
    if (is_inf(p)) {
        set_affine(p, x2, y2);
        return MADD_DONE;
    }
    const F2 Z1Z1 = sqr(p.z);
    const F2 U2 = mul(x2, Z1Z1), S2 = mul(mul(y2, p.z), Z1Z1);
    const F2 H = sub<4>(U2, p.x), r = sub<4>(S2, p.y);
    if (is_zero(H)) {
        if (is_zero(r)) return MADD_DOUBLE;
        set_inf(p);
        return MADD_INF;
    }
    const F2 I = dbl(dbl(sqr(H)));
    const F2 J = mul(H, I), V = mul(p.x, I);
    const F2 rr4 = dbl(dbl(sqr(r)));
    const F2 X3 = red(sub<32>(rr4, add(J, dbl(V))));
    const F2 Y3 = red(sub<32>(mul(dbl(r), sub<4>(V, X3)), dbl(mul(p.y, J))));
    p.z = mul(dbl(p.z), H);
    p.x = X3;
    p.y = Y3;
    return MADD_DONE;
}
// the complete addition: p += (x2, y2) whatever the two points are
FF_HD void madd_complete(Jac& p, const F2& x2, const F2& y2) {
    if (madd(p, x2, y2) == MADD_DOUBLE) dbl(p);
}

// p += q, two Jacobian points, complete in both operands (add-2007-bl, the value of pairing::g2_add; P + P is dbl(p)
// as there, P - P is infinity, an operand at infinity gives the other).  X, Y < 3 and Z < 10 on both sides.
//   Z1Z1, Z2Z2 < 4; U1 = X1 Z2Z2, U2 = X2 Z1Z1: 3 * 4, < 10; S1 = (Y1 Z2) Z2Z2, S2 = (Y2 Z1) Z1Z1: 3 * 10, then
//   10 * 4, < 10; U1 and S1 reduced: < 2 (they are subtracted, and multiplied again below);
//   H = U2 + 4p - U1 < 14, r = S2 + 4p - S1 < 14; both zero-tested (< 2^6);
//   I = (2H)^2 = 4 H^2 < 16 (H < 15, H^2 < 4); J = H I: 14 * 16, < 10; V = U1 I: 2 * 16, < 10;
//   (2r)^2 = 4 r^2 < 16; J + 2V < 30 <= 31: X3 = 4r^2 + 32p - J - 2V < 48, reduced: < 2;
//   (2r)(V + 4p - X3): 28 * 14 <= 630, < 10; 2 S1 J: S1 J is 2 * 10, < 10, doubled < 20 <= 31: Y3 < 42, reduced: < 2;
//   Z3 = ((Z1 + Z2)^2 - Z1Z1 - Z2Z2) H = ((2 Z1) Z2) H: 20 * 10, < 10, then 10 * 14, < 10.
// The doubling inside takes X, Y < 15, Z < 21.
FF_HD void add(Jac& p, const Jac& q) {
    if (is_inf(q)) return;
    if (is_inf(p)) {
        p = q;
        return;
    }
    const F2 Z1Z1 = sqr(p.z), Z2Z2 = sqr(q.z);
    const F2 U1 = red(mul(p.x, Z2Z2)), U2 = mul(q.x, Z1Z1);
    const F2 S1 = red(mul(mul(p.y, q.z), Z2Z2)), S2 = mul(mul(q.y, p.z), Z1Z1);
    const F2 H = sub<4>(U2, U1), r = sub<4>(S2, S1);
    if (is_zero(H)) {
        if (is_zero(r)) dbl(p);
        else set_inf(p);
        return;
    }
    const F2 I = dbl(dbl(sqr(H)));
    const F2 J = mul(H, I), V = mul(U1, I);
    const F2 rr4 = dbl(dbl(sqr(r)));
    const F2 X3 = red(sub<32>(rr4, add(J, dbl(V))));
    const F2 Y3 = red(sub<32>(mul(dbl(r), sub<4>(V, X3)), dbl(mul(S1, J))));
    p.z = mul(mul(dbl(p.z), q.z), H);
    p.x = X3;
    p.y = Y3;
}

// One step of a table walk: p += e for neg == 0, p -= e otherwise, e a table entry (canonical x, y, or flagged as
// infinity: then p is left alone).  Complete in both operands: this is what the walk of a base outside the subgroup
// relies on, where entries are infinite and P + P and P - P occur.  Bounds as madd (-e is neg<2>(y) <= 2).
FF_HD void madd_tab(Jac& p, const AffPt& e, u32 neg_mask) {
    if (e.flags & 1) return;
    madd_complete(p, e.x, neg_mask ? neg<2>(e.y) : e.y);
}

// (X / Z^2, Y / Z^3) as canonical residues (pairing::g2_to_affine); infinity: flags = 1, x = y = 0.  X, Y, Z < 15.
FF_HD void to_affine(AffPt& out, const Jac& p) {
    out.pad[0] = out.pad[1] = out.pad[2] = 0;
    if (is_inf(p)) {
        out.x = out.y = zero();
        out.flags = 1;
        return;
    }
    const F2 zi = inv(p.z), zi2 = sqr(zi);
    const F2 x = red(mul(p.x, zi2)), y = red(mul(p.y, mul(zi2, zi)));
    out.x = {fp28::canon(x.c0), fp28::canon(x.c1)};
    out.y = {fp28::canon(y.c0), fp28::canon(y.c1)};
    out.flags = 0;
}

// blst_p2 layout: six Fp (x.c0, x.c1, y.c0, y.c1, z.c0, z.c1), Montgomery 2^384; infinity <=> Z == 0
FF_HD void from_blst_jacobian(Jac& p, const ff::Fp in[6]) {
    if (in[4].is_zero() && in[5].is_zero()) {
        set_inf(p);
        return;
    }
    p.x = from_blst(in);
    p.y = from_blst(in + 2);
    p.z = from_blst(in + 4);
}
FF_HD void to_blst_jacobian(ff::Fp out[6], const Jac& p) {  // canonical residues; infinity -> all-zero
    if (is_inf(p)) {
#pragma unroll
        for (int i = 0; i < 6; ++i) out[i] = ff::Fp::zero();
        return;
    }
    to_blst(out, p.x);
    to_blst(out + 2, p.y);
    to_blst(out + 4, p.z);
}

}  // namespace g2
