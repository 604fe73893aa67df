// G1 wire format on the device: ZCash-compressed 48-byte points <-> fp28 coordinates.
// Replaces what the reference gets from blst_p1_uncompress / blst_p1_compress through
// FsG1::from_bytes / to_bytes (blst/src/types/g1.rs:65-100); flag semantics as stated
// in-tree at zkcrypto/bls12_381/src/g1.rs:337-392.
// Also the single-lane membership test of a decoded point (affpt_in_g1), so that the host-compiled tests reach it.
#pragma once
#include "g1_28.hip.h"

namespace g1io {
using ff::u32;
using ff::u64;
using fp28::Fe;

FF_HD constexpr u32 r2_392_l(int i) {  // 2^784 mod p
    constexpr u32 t[14] = {0x10370edu, 0x6d1c345u, 0xe243d62u, 0xec45c53u, 0x3b1d65au, 0x93317du, 0xb4f36a0u,
                           0x5d74088u, 0xc10ea72u, 0x865d118u, 0x7320a75u, 0xfd5cd50u, 0xcc8a759u, 0xc8d4u};
    return t[i];
}
FF_HD constexpr u32 b4_392_l(int i) {  // 4 * 2^392 mod p  (curve constant b = 4)
    constexpr u32 t[14] = {0xd1ff2e0u, 0x6000000u, 0xac467u, 0x3379b48u, 0x1c84b80u, 0xe88243u, 0xdd9a7eu,
                           0x683dcf8u, 0x6c26d0bu, 0x4a5eec2u, 0x457663cu, 0x4b29f1u, 0x967f3e8u, 0x15de9u};
    return t[i];
}
FF_HD constexpr u32 p_half_l(int i) {  // (p-1)/2, saturated limbs
    constexpr u32 t[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u,
                           0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};
    return t[i];
}
FF_HD constexpr u32 p_sqrt_exp_l(int i) {  // (p+1)/4, saturated limbs
    constexpr u32 t[12] = {0xffffeaabu, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                           0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};
    return t[i];
}

// plain (non-Montgomery) canonical integer of a field element
FF_HD ff::Fp to_plain(const Fe& a) {
    Fe one_raw = fp28::zero();
    one_raw.v[0] = 1;
    ff::Fp s = fp28::pack(fp28::mul(a, one_raw));
    ff::reduce_once(s);
    return s;
}
// plain canonical integer (< p) -> Montgomery-392
FF_HD Fe from_plain(const ff::Fp& a) {
    Fe c;
#pragma unroll
    for (int i = 0; i < 14; ++i) c.v[i] = r2_392_l(i);
    return fp28::mul(fp28::unpack(a), c);
}

FF_HD bool sat_geq_p(const ff::Fp& a) {
    u64 borrow = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        u64 d = (u64)a.v[i] - ff::FpParams::p(i) - borrow;
        borrow = (d >> 32) & 1;
    }
    return borrow == 0;
}
FF_HD bool is_lex_largest(const ff::Fp& plain) {  // plain > (p-1)/2
    u64 borrow = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        u64 d = (u64)p_half_l(i) - plain.v[i] - borrow;
        borrow = (d >> 32) & 1;
    }
    return borrow != 0;
}

template <class ExpFn>
FF_HD Fe pow_sat(const Fe& a, ExpFn e) {
    Fe r = fp28::one();
    bool started = false;
    for (int i = 11; i >= 0; --i) {
        const u32 w = e(i);
        for (int b = 31; b >= 0; --b) {
            if (started) r = fp28::sqr(r);
            if ((w >> b) & 1) {
                r = started ? fp28::mul(r, a) : a;
                started = true;
            }
        }
    }
    return r;
}
FF_HD Fe inverse_fermat(const Fe& a) {
    return pow_sat(a, [](int i) -> u32 { return i == 0 ? ff::FpParams::p(0) - 2 : ff::FpParams::p(i); });
}
// a^-1 in the 2^392 Montgomery domain via the (batched) binary-Euclid inverse of the plain residue:
// (x*R')^-1 = x^-1 * R'^-1, then two multiplications by R'^2 give x^-1 * R'
FF_HD Fe inverse(const Fe& a) {
    ff::Fp s = fp28::pack(a);  // normalized, value < 2^384 (callers pass mul outputs, < 2p)
    ff::reduce_once(s);
    ff::reduce_once(s);
    const ff::Fp inv = ff::inverse_plain_fast(s);
    Fe c;
#pragma unroll
    for (int i = 0; i < 14; ++i) c.v[i] = r2_392_l(i);
    return fp28::mul(fp28::mul(fp28::unpack(inv), c), c);
}

// 48 big-endian bytes -> saturated plain integer
FF_HD ff::Fp be48_to_sat(const unsigned char* in) {
    ff::Fp r;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const unsigned char* q = in + (11 - i) * 4;
        r.v[i] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
    }
    return r;
}
FF_HD void sat_to_be48(unsigned char* out, const ff::Fp& a) {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        unsigned char* q = out + (11 - i) * 4;
        q[0] = (unsigned char)(a.v[i] >> 24);
        q[1] = (unsigned char)(a.v[i] >> 16);
        q[2] = (unsigned char)(a.v[i] >> 8);
        q[3] = (unsigned char)a.v[i];
    }
}

// blst_p1_uncompress: returns false on an invalid encoding.  On-curve by construction,
// no subgroup check (same as FsG1::from_bytes).  Infinity -> flags bit0.
FF_HD bool uncompress(g1::AffPt& out, const unsigned char in[48]) {
    out.flags = 0;
    out.pad[0] = out.pad[1] = out.pad[2] = 0;
    out.x = fp28::zero();
    out.y = fp28::zero();
    const bool compressed = (in[0] >> 7) & 1, infinity = (in[0] >> 6) & 1, sort = (in[0] >> 5) & 1;
    if (!compressed) return false;
    unsigned char tmp[48];
    for (int i = 0; i < 48; ++i) tmp[i] = in[i];
    tmp[0] &= 0x1f;
    ff::Fp xs = be48_to_sat(tmp);
    if (infinity) {
        if (sort || !xs.is_zero()) return false;
        out.flags = 1;
        return true;
    }
    if (sat_geq_p(xs)) return false;
    Fe x = from_plain(xs);
    Fe b4;
#pragma unroll
    for (int i = 0; i < 14; ++i) b4.v[i] = b4_392_l(i);
    Fe y2 = fp28::addn(fp28::mul(fp28::sqr(x), x), b4);  // x^3 + 4, < 4p
    Fe y = pow_sat(y2, [](int i) -> u32 { return p_sqrt_exp_l(i); });
    // is it a root?
    Fe chk = fp28::sub<8>(fp28::sqr(y), y2);
    if (!fp28::is_zero_mod_p(chk)) return false;
    y = fp28::canon(y);
    if (is_lex_largest(to_plain(y)) != sort) y = fp28::canon(fp28::neg<2>(y));
    out.x = fp28::canon(x);
    out.y = y;
    return true;
}

// blst_p1_compress of an XYZZ point, given zi = 1 / (ZZ * ZZZ)
FF_HD void compress_with_inverse(unsigned char out[48], const g1::Xyzz& p, const Fe& zi) {
    if (g1::is_inf(p)) {
        for (int i = 0; i < 48; ++i) out[i] = 0;
        out[0] = 0xc0;
        return;
    }
    Fe x = fp28::mul(p.x, fp28::mul(zi, p.zzz));
    Fe y = fp28::mul(p.y, fp28::mul(zi, p.zz));
    sat_to_be48(out, to_plain(x));
    out[0] |= 0x80;
    if (is_lex_largest(to_plain(y))) out[0] |= 0x20;
}
FF_HD void compress(unsigned char out[48], const g1::Xyzz& p) {
    Fe zi = fp28::one();
    if (!g1::is_inf(p)) zi = inverse(fp28::mul(p.zz, p.zzz));
    compress_with_inverse(out, p, zi);
}

// One lane's share of a batched blst_p1_compress / blst_p1_to_affine (codec.hip): m <= CH Jacobian points in the blst_p1
// layout (three Fp each, Montgomery 2^384, canonical; the identity is Z all-zero, whatever X and Y hold) with ONE
// inversion, by Montgomery's trick over the non-zero Z of the chunk, as host_p1_compress_batch / host_p1_to_affine_batch
// do it on the host.  AFFINE: out is blst_p1_affine[m] (two Fp per point, the identity as (0, 0)); otherwise 48 bytes per
// point.  A chunk of 0 points, of 1 point and of identities only is handled (the inversion then runs on one).
// Every operand is a product's output (< 2p): the running product, the prefixes, z^-1, x and y.  The loops are kept
// rolled: the prefixes are indexed by the loop counter (scratch on the device) and the body is eight products long.
template <int CH, bool AFFINE>
FF_HD void jac_chunk_out(void* out, const ff::Fp* jac, int m) {
    Fe pre[CH];
    Fe run = fp28::one();
#pragma unroll 1
    for (int i = 0; i < m; ++i) {
        pre[i] = run;
        if (!jac[3 * i + 2].is_zero()) run = fp28::mul(run, fp28::from_blst(jac[3 * i + 2]));
    }
    Fe inv = m > 0 ? inverse(run) : run;
#pragma unroll 1
    for (int i = m - 1; i >= 0; --i) {
        const bool inf = jac[3 * i + 2].is_zero();
        Fe x = fp28::zero(), y = fp28::zero();
        if (!inf) {
            const Fe zi = fp28::mul(inv, pre[i]), zi2 = fp28::sqr(zi);
            inv = fp28::mul(inv, fp28::from_blst(jac[3 * i + 2]));
            x = fp28::mul(fp28::from_blst(jac[3 * i]), zi2);
            y = fp28::mul(fp28::from_blst(jac[3 * i + 1]), fp28::mul(zi2, zi));
        }
        if (AFFINE) {
            ff::Fp* o = (ff::Fp*)out + 2 * i;
            o[0] = inf ? ff::Fp::zero() : fp28::to_blst(x);
            o[1] = inf ? ff::Fp::zero() : fp28::to_blst(y);
        } else {
            unsigned char* o = (unsigned char*)out + 48 * i;
            if (inf) {
                for (int k = 0; k < 48; ++k) o[k] = 0;
                o[0] = 0xc0;
            } else {
                sat_to_be48(o, to_plain(x));
                o[0] |= 0x80;
                if (is_lex_largest(to_plain(y))) o[0] |= 0x20;
            }
        }
    }
}

// the r-torsion test of a decoded point: phi(P) == -[x^2]P, phi(x,y) = (beta*x, y), x the BLS parameter (the in-tree
// statement of the same test: zkcrypto/bls12_381/src/g1.rs:401-435).  Two 64-bit scalar multiplications instead of one
// by the 255-bit group order.
FF_HD bool affpt_in_g1(const g1::AffPt& p) {
    if (p.flags & 1) return true;
    const unsigned long long BLS_X = 0xd201000000010000ull;  // |x|; the sign cancels in x^2
    g1::Xyzz q1, q2;
    g1::set_inf(q1);
    for (int bit = 63; bit >= 0; --bit) {
        if (!g1::is_inf(q1)) g1::dbl(q1);
        if ((BLS_X >> bit) & 1) g1::madd(q1, p.x, p.y);
    }
    g1::set_inf(q2);
    for (int bit = 63; bit >= 0; --bit) {
        if (!g1::is_inf(q2)) g1::dbl(q2);
        if ((BLS_X >> bit) & 1) g1::dadd(q2, q1);
    }
    if (g1::is_inf(q2)) return false;
    fp28::Fe beta;
    {
        constexpr u32 t[14] = {0xa75929au, 0x681b798u, 0x22a3e9du, 0xabc02bfu, 0x4e5bb45u, 0x55e6e7eu, 0x4814117u,
                               0x6d04f1bu, 0xae3387du, 0x54acb0cu, 0xa4c74bu, 0x56138b5u, 0xb64e066u, 0x76f2u};
#pragma unroll
        for (int k = 0; k < 14; ++k) beta.v[k] = t[k];  // cube root of unity, Montgomery 2^392
    }
    // phi(P) == -Q2  <=>  beta*x*ZZ == X  and  y*ZZZ == -Y
    const fp28::Fe dx = fp28::sub<16>(fp28::mul(fp28::mul(beta, p.x), q2.zz), q2.x);
    const fp28::Fe dy = fp28::addn(fp28::mul(p.y, q2.zzz), q2.y);
    return fp28::is_zero_mod_p(dx) && fp28::is_zero_mod_p(dy);
}

}  // namespace g1io
