// The per-lane part of a G2 linear combination (setupcheck.hip), host- and device-compilable so that
// tests/test_g2_add_cpu.py runs the very walk the kernel runs against host_pairing.h: one term k * P by a left-to-right
// double-and-add over the affine form of P, and the pairwise tree that sums 64 terms.  tests/test_g2_arith_gpu.py runs
// term (one point and scalar per lane) and tree_step (the 64 slots in LDS) on the device against Python integers.  Only
// routines of g2_28.hip.h, inside the bounds its table states:
//   from_blst_jacobian  X, Y, Z < 2 (products)             -> to_affine takes X, Y, Z < 15; x, y canonical
//   the walk            acc is the affine point (canonical, Z = one), or what dbl (X, Y < 2, Z < 10) or madd
//                       (X, Y < 3, Z < 10) left: dbl takes X, Y < 15, Z < 21, madd X1, Y1 < 3, Z1 < 10
//   the tree            operands are terms (X, Y < 3, Z < 10) or sums (X, Y < 2, Z < 10): add takes X, Y < 3, Z < 10
#pragma once
#include "ff.hip.h"
#include "g2_28.hip.h"

namespace g2lc {

constexpr int LANES = 64;  // terms per workgroup, and operands per launch of the sum kernel

// acc = k * P: P a blst_p2 (canonical coordinates, any Z; Z == 0 the identity), k a Montgomery blst_fr.  An infinite
// point or a zero scalar gives infinity.  256 steps whatever k is; the doublings before the top set bit are skipped by
// the infinity test (which also carries a P outside the subgroup through k's multiples of its order).
FF_HD void term(g2::Jac& acc, const ff::Fp pt[6], const ff::Fr& k_mont) {
    g2::set_inf(acc);
    g2::AffPt a;
    {
        g2::Jac p;
        g2::from_blst_jacobian(p, pt);
        g2::to_affine(a, p);
    }
    const ff::Fr k = ff::from_mont(k_mont);
    if ((a.flags & 1) || k.is_zero()) return;
#pragma unroll 1
    for (int bit = 255; bit >= 0; --bit) {
        if (!g2::is_inf(acc)) g2::dbl(acc);
        if ((k.v[bit >> 5] >> (bit & 31)) & 1) g2::madd_complete(acc, a.x, a.y);
    }
}

// one level of the tree over slots[0 .. 2 * half): slot t += slot t + half, for the lane t < half that calls it
FF_HD void tree_step(g2::Jac* slots, int t, int half) {
    g2::Jac a = slots[t];
    g2::add(a, slots[t + half]);
    slots[t] = a;
}

}  // namespace g2lc
