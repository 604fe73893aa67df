// G2 wire format and membership on the device, one value per lane: ZCash-compressed 96-byte points <-> g2::AffPt /
// g2::Jac, in the style of g1_io.hip.h.  host_pairing.h is the specification (f2_sqrt up to the sign of the root,
// f2_lex_largest, g2_uncompress, g2_compress, g2_in_g2); tests/test_point_codec_cpu.py compiles this header for the
// host and compares every routine with it and with tests/codec_model.py; tests/test_g2_arith_gpu.py runs every routine
// of the table below on the device, one value per lane, against tests/codec_model.py (cases in tests/g2_lane_cases.py).
//
// Bounds, in the language of g2_28.hip.h ("a < K": both components normalized with value < K*p):
//
//   routine            accepts                          returns
//   canon2(a)          an Fe, normalized, <= 2p         the canonical residue (fp28::canon gives p for 2p)
//   lex_largest(y)     y < 2520 (a product's operand)   the sign flag of y: exact
//   sqrt(out, a)       a < 2^6                          true and out < 2 with out^2 == a, or false: a is no square
//   uncompress         96 bytes                         canonical x, y (or the infinity flag); false: no encoding
//   compress           X, Y, Z < 15 (or Z all-zero)     96 bytes
//   psi(P)             canonical x, y                   x, y < 2 (not canonical)
//   in_g2(P)           canonical x, y (or flagged)      exact
//
// sqrt, the norm form: for a = a0 + a1 u with norm n = a0^2 + a1^2, s = sqrt(n) in Fp exists iff a is a square of Fp2.
// A root x0 + x1 u has x0^2 - x1^2 = a0 and 2 x0 x1 = a1, so 4 x0^2 = 2 (a0 +- s) =: t; the two choices of the sign
// multiply to -4 a1^2, so exactly one of them is a square of Fp when a1 != 0, and c = t^((p+1)/4) has c^2 = t or
// c^2 = -t (p = 3 mod 4).  With w = 1 / (2c):
//     c^2 ==  t:  x = (t w, 2 a1 w)         (x0 = c / 2, x1 = a1 / c)
//     c^2 == -t:  x = (2 a1 w, -t w)        (x0 = a1 / c, x1 = c / 2 = -t / (2c))
// t == 0 (a1 == 0 and s == -a0) takes the other sign of s, t = 4 a0.  Two Fp exponentiations and one inversion instead
// of the two Fp2 exponentiations of pairing::f2_sqrt; the result is confirmed by squaring, so which root-finding
// algorithm runs cannot change a verdict, and the sign is fixed afterwards by the flag.
//   a reduced: < 2; n = a0^2 + a1^2 < 4 (an operand of pow_sat as x^3 + 4 is in g1io::uncompress); s < 2;
//   s^2 + 8p - n: n < 7; t = 2 (a0 + s) < 8 (or 2 (a0 + 4p - s) < 12), reduced: < 2; c < 2; c^2 + 4p - t: t < 3;
//   2c < 4, reduced for g1io::inverse (a product's output); 2 a1 < 4, -t = 4p - t <= 4: products of < 4 by < 2;
//   x^2 + 4p - a: x^2 has c0 < 2, c1 < 4, a < 3: the zero test sees < 8.
//
// in_g2: psi(P) == [x]P for the (negative) BLS parameter x, i.e. psi(P) == -[|x|]P, psi = twist o Frobenius o untwist
// = (conj(x) / xi^((p-1)/3), conj(y) / xi^((p-1)/2)), xi = 1 + u.  Sufficient for membership on BLS12 curves: M. Scott,
// "A note on group membership tests for G1, G2 and GT on BLS pairing-friendly curves", ePrint 2021/1130, section 4.
// The two constants are derived in tests/codec_model.py (psi_constants) and the limbs below are compared with them
// there; the real part of the first is zero.  [|x|]P is 63 doublings and 5 complete additions (g2::dbl: X, Y < 15,
// Z < 21 in, X, Y < 2, Z < 10 out; g2::madd: X, Y < 3, Z < 10 in and out); the group E'(Fp2) has odd order, so no
// doubling of a point other than infinity gives infinity.  The comparison is projective: px Z^2 == X, py Z^3 == -Y
// (px, py < 2; Z^2: c1 < 4; Z^3 = Z^2 Z: 4 * 10 <= 630, < 10; px Z^2 + 4p - X < 14, py Z^3 + Y < 13).
#pragma once
#include "g1_io.hip.h"
#include "g2_28.hip.h"

namespace g2io {
using ff::u32;
using fp28::Fe;
using g2::F2;

FF_HD constexpr u32 psi_x_c1_l(int i) {  // imaginary part of 1 / xi^((p-1)/3), Montgomery 2^392 (the real part is 0)
    constexpr u32 t[14] = {0x58a1811u, 0x96e4867u, 0x1d5c11cu, 0x543e856u, 0x13e6366u, 0x4b0fc91u, 0xae5efbbu,
                           0x8680210u, 0x9941307u, 0xf700269u, 0xb02eef7u, 0x9086bfcu, 0x6855919u, 0x1291eu};
    return t[i];
}
FF_HD constexpr u32 psi_y_c0_l(int i) {  // 1 / xi^((p-1)/2), real part
    constexpr u32 t[14] = {0xcc17b84u, 0xcc5da55u, 0x1835de7u, 0x3e1e677u, 0x9e4ae31u, 0x9b9a07au, 0xd662557u,
                           0xb7f1997u, 0x71cc4dau, 0xa667f92u, 0x65115feu, 0x4a3370cu, 0xe5b746au, 0xd16du};
    return t[i];
}
FF_HD constexpr u32 psi_y_c1_l(int i) {  // 1 / xi^((p-1)/2), imaginary part
    constexpr u32 t[14] = {0x33e2f27u, 0x32a25aau, 0x27ca1d2u, 0xc1e049eu, 0xc3f707au, 0x55ca94u, 0x2010b7bu,
                           0x3b93794u, 0xd5a86aau, 0xa544de3u, 0x556a044u, 0x9c66da5u, 0x38ec515u, 0xcea3u};
    return t[i];
}
FF_HD F2 psi_x() {
    F2 c = g2::zero();
#pragma unroll
    for (int i = 0; i < 14; ++i) c.c1.v[i] = psi_x_c1_l(i);
    return c;
}
FF_HD F2 psi_y() {
    F2 c;
#pragma unroll
    for (int i = 0; i < 14; ++i) {
        c.c0.v[i] = psi_y_c0_l(i);
        c.c1.v[i] = psi_y_c1_l(i);
    }
    return c;
}

// canonical residue of a normalized value <= 2p
FF_HD Fe canon2(const Fe& a) {
    ff::Fp s = fp28::pack(a);
    ff::reduce_once(s);
    ff::reduce_once(s);
    return fp28::unpack(s);
}

// pairing::f2_lex_largest: the imaginary part decides, the real part when the imaginary part is zero
FF_HD bool lex_largest(const F2& y) {
    const ff::Fp c1 = g1io::to_plain(y.c1);
    if (!c1.is_zero()) return g1io::is_lex_largest(c1);
    return g1io::is_lex_largest(g1io::to_plain(y.c0));
}

FF_HD Fe sqrt_exp(const Fe& a) {  // a^((p+1)/4)
    return g1io::pow_sat(a, [](int i) -> u32 { return g1io::p_sqrt_exp_l(i); });
}

// some square root of a, or false (the table and the derivation above)
FF_HD bool sqrt(F2& out, const F2& a_in) {
    const F2 a = g2::red(a_in);
    out = g2::zero();
    if (g2::is_zero(a)) return true;
    const Fe n = fp28::addn(fp28::sqr(a.c0), fp28::sqr(a.c1));
    const Fe s = sqrt_exp(n);
    if (!fp28::is_zero_mod_p(fp28::sub<8>(fp28::sqr(s), n))) return false;  // the norm is no square: neither is a
    Fe t = fp28::addn(a.c0, s);
    t = fp28::addn(t, t);
    if (fp28::is_zero_mod_p(t)) {
        t = fp28::sub<4>(a.c0, s);
        t = fp28::addn(t, t);
    }
    t = fp28::mul(t, fp28::one());
    const Fe c = sqrt_exp(t);
    if (fp28::is_zero_mod_p(c)) return false;  // t != 0 here for a != 0: never, and the inversion needs it
    const bool plus = fp28::is_zero_mod_p(fp28::sub<4>(fp28::sqr(c), t));
    const Fe w = g1io::inverse(fp28::mul(fp28::addn(c, c), fp28::one()));
    const Fe a1x2 = fp28::addn(a.c1, a.c1);
    F2 x;
    if (plus) x = {fp28::mul(t, w), fp28::mul(a1x2, w)};
    else x = {fp28::mul(a1x2, w), fp28::mul(fp28::neg<4>(t), w)};
    if (!g2::is_zero(g2::sub<4>(g2::sqr(x), a))) return false;
    out = x;
    return true;
}

// pairing::g2_uncompress: false on an invalid encoding; on the curve by construction, no subgroup test.
// Infinity -> flags bit0, x = y = 0.
FF_HD bool uncompress(g2::AffPt& out, const unsigned char in[96]) {
    out.flags = 0;
    out.pad[0] = out.pad[1] = out.pad[2] = 0;
    out.x = out.y = g2::zero();
    const bool compressed = (in[0] >> 7) & 1, infinity = (in[0] >> 6) & 1, sort = (in[0] >> 5) & 1;
    if (!compressed) return false;
    unsigned char tmp[48];
    for (int i = 0; i < 48; ++i) tmp[i] = in[i];
    tmp[0] &= 0x1f;
    const ff::Fp x1s = g1io::be48_to_sat(tmp), x0s = g1io::be48_to_sat(in + 48);
    if (infinity) {
        if (sort || !x1s.is_zero() || !x0s.is_zero()) return false;
        out.flags = 1;
        return true;
    }
    if (g1io::sat_geq_p(x1s) || g1io::sat_geq_p(x0s)) return false;
    const F2 x = {g1io::from_plain(x0s), g1io::from_plain(x1s)};
    F2 b;
#pragma unroll
    for (int i = 0; i < 14; ++i) b.c0.v[i] = b.c1.v[i] = g1io::b4_392_l(i);  // 4 (1 + u)
    const F2 y2 = g2::add(g2::mul(g2::sqr(x), x), b);  // c0 < 7, c1 < 11
    F2 y;
    if (!sqrt(y, y2)) return false;
    y = {fp28::canon(y.c0), fp28::canon(y.c1)};
    if (lex_largest(y) != sort) y = {canon2(fp28::neg<2>(y.c0)), canon2(fp28::neg<2>(y.c1))};
    out.x = {fp28::canon(x.c0), fp28::canon(x.c1)};
    out.y = y;
    return true;
}

// pairing::g2_compress of a Jacobian point (the inversion is g2::inv, through g2::to_affine)
FF_HD void compress(unsigned char out[96], const g2::Jac& p) {
    g2::AffPt a;
    g2::to_affine(a, p);
    if (a.flags & 1) {
        for (int i = 0; i < 96; ++i) out[i] = 0;
        out[0] = 0xc0;
        return;
    }
    g1io::sat_to_be48(out, g1io::to_plain(a.x.c1));
    g1io::sat_to_be48(out + 48, g1io::to_plain(a.x.c0));
    out[0] |= 0x80;
    if (lex_largest(a.y)) out[0] |= 0x20;
}

// the endomorphism on an affine point not at infinity; x, y canonical in, < 2 out
FF_HD void psi(F2& px, F2& py, const F2& x, const F2& y) {
    const F2 cx = {x.c0, fp28::neg<2>(x.c1)}, cy = {y.c0, fp28::neg<2>(y.c1)};
    px = g2::red(g2::mul(cx, psi_x()));
    py = g2::red(g2::mul(cy, psi_y()));
}

// P in G2 (infinity included): psi(P) == -[|x|]P
FF_HD bool in_g2(const g2::AffPt& p) {
    if (p.flags & 1) return true;
    const unsigned long long BLS_X = 0xd201000000010000ull;  // |x|
    g2::Jac q;
    g2::set_inf(q);
    for (int bit = 63; bit >= 0; --bit) {
        if (!g2::is_inf(q)) g2::dbl(q);
        if ((BLS_X >> bit) & 1) g2::madd_complete(q, p.x, p.y);
    }
    if (g2::is_inf(q)) return false;  // the order of P divides |x| < r
    F2 px, py;
    psi(px, py, p.x, p.y);
    const F2 zz = g2::sqr(q.z), zzz = g2::mul(zz, q.z);
    const F2 dx = g2::sub<4>(g2::mul(px, zz), q.x);
    const F2 dy = g2::add(g2::mul(py, zzz), q.y);
    return g2::is_zero(dx) && g2::is_zero(dy);
}

}  // namespace g2io
