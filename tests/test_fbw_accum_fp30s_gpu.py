"""k_fbw_accum over fp30s (g1_30s.hip.h: 13 signed 30-bit limbs, the chain on the isomorphic curve the table's integers
are a point of in that radix) against the oracle's MSM, byte for byte.

Prepared MSMs over n = 64 random bases with a small wide table, in the batch sizes that reach each instantiation
msm_enqueue picks for them: batches of 3 (one scalar group per lane: k_fbw_accum<2, true> with the GLV split,
<1, false> without) and of 256 (four scalars per lane: <8, true> / <4, false>); the form without the split over bases
outside G1, where the handle chooses it itself; and one segmented handle (MatrixMsm, 4 rows of 64 table bases): as
msm_enqueue sizes it (one scalar group per lane again, <2, true>) and with the tuning key `spl` at 8 and 16, which is
what msm_enqueue picks for segment MSMs from 2^20 and 2^21 scalars per call on: k_fbw_accum<16, true> and <32, true>.
The form without the split also runs with `spl` = 2 (<2, false>, which msm_enqueue never picks by itself).  Not reached
here: <1, true>, which takes a few MSMs over exactly 4096 bases (test_fbw_accum_chain_start_gpu.py does not reach it
either; the 4096-point suites do).
Scalars: 0, 1, r - 1; every window at the digit 2^(c-1), at 2^(c-1) + 1 (a negative digit and a carry in every
window) and all ones (a carry through all windows), in the k1 half, the k2 half and both; one base repeated with equal
and with opposite scalars next to each other, so that a chain meets P + P and P - P; random scalars."""
import ctypes as C
import random

import pytest

import oracle_ffi as O
from test_msm_gpu import as_oracle_g1, compressed, curve_points_outside_g1, gen_points

pytestmark = pytest.mark.gpu

N = 64
X2 = 0xD201000000010000 ** 2  # k = k1 + k2 * X2 (glv.hip.h)
INF = b"\xc0" + bytes(47)


def window_patterns(c):
    """126-bit values (the GLV split leaves them whole in one half)"""
    nw = 126 // c
    half = 1 << (c - 1)
    return [sum(half << (c * w) for w in range(nw)),
            sum((half + 1) << (c * w) for w in range(nw)),
            (1 << (c * nw)) - 1]


def patterns(c, seed, repeated):
    """[(name, 64 scalars)]; `repeated`: bases 8..11 are one point"""
    rnd = random.Random(seed)
    pats = [("zero_one_rminus1", [(0, 1, O.R - 1)[i % 3] for i in range(N)])]
    for k, v in enumerate(window_patterns(c)):
        pats.append(("windows%d_k1" % k, [v] * N))
        pats.append(("windows%d_k2" % k, [v * X2 % O.R] * N))
        pats.append(("windows%d_both_neg" % k, [(O.R - (v + v * X2)) % O.R] * N))
    for k in range(2):
        v = [rnd.randrange(O.R) for _ in range(N)]
        s = rnd.randrange(1, O.R)
        if repeated:
            v[8], v[9], v[10], v[11] = s, s, O.R - s, s   # P + P, then 2P - P, then P + P again in one chain
        pats.append(("repeated%d" % k, v))
    for k in range(3):
        pats.append(("random%d" % k, [rnd.randrange(O.R) for _ in range(N)]))
    return pats


def bases(L, seed, outside=False):
    pts = gen_points(L, N, random.Random(seed))
    for i in (9, 10, 11):
        pts[i] = pts[8]
    if outside:
        for (x, y), i in zip(curve_points_outside_g1(2, 77), (3, 40)):
            pts[i].x, pts[i].y = O.fp_from_int(x), O.fp_from_int(y)
    return pts


def expected(L, pts, pats):
    out = []
    for _, v in pats:
        e = O.G1()
        L.omsm_naive(C.byref(e), pts, O.fr_array(v), N)
        out.append(compressed(L, e))
    return out


@pytest.mark.parametrize("form", ["glv", "plain", "plain_spl2", "outside_g1"])
def test_prepared_batches_against_the_oracle(oracle, kzg, form):
    L = oracle.lib()
    pts = bases(L, 0x30A, outside=form == "outside_g1")
    cfg = kzg.make_config(table_budget_gb=0.25, tuning={"plain": {"fbw_glv": 0}, "plain_spl2": {"fbw_glv": 0, "spl": 2}}.get(form, {}))
    h = kzg.prepare_multi_scalar_mult(pts, N, cfg)
    try:
        info = h.info()
        assert info["wide_table"] and info["wide_glv"] == (form == "glv"), info
        pats = patterns(info["window_bits"], 64, repeated=True)
        want = expected(L, pts, pats)
        assert len(set(want)) > len(want) - 3
        for nbatch in (3, 256):
            for first in range(0, len(pats), nbatch):
                idx = [(first + j) % len(pats) for j in range(nbatch)]
                sc = O.fr_array([s for i in idx for s in pats[i][1]])
                got = kzg.multi_scalar_mult_prepared_batch(h, sc, N, nbatch)
                bad = [pats[i][0] for b, i in enumerate(idx) if compressed(L, as_oracle_g1(got[b])) != want[i]]
                assert not bad, (nbatch, bad)
    finally:
        h.close()


@pytest.mark.parametrize("tuning", [{}, {"spl": 8}, {"spl": 16}], ids=["spl=auto", "spl=8", "spl=16"])
def test_a_segmented_handle_against_the_oracle(oracle, kzg, tuning):
    L = oracle.lib()
    rows = 4
    per_row = [bases(L, 0x30B + r) for r in range(rows)]
    flat = (O.G1Affine * (rows * N))(*[p for r in per_row for p in r[:N]])
    h = kzg.MatrixMsm(flat, rows, N, kzg.make_config(table_budget_gb=0.25, tuning=tuning))
    try:
        info = h.info()
        assert info["wide_table"] and info["wide_glv"], info
        pats = patterns(info["window_bits"], 65, repeated=True)
        nmat = (len(pats) + rows - 1) // rows
        idx = [k % len(pats) for k in range(nmat * rows)]  # MSM k runs over the bases of row k % rows
        want = {}
        for k, i in enumerate(idx):
            want[k] = expected(L, per_row[k % rows], [pats[i]])[0]
        sc = O.fr_array([s for i in idx for s in pats[i][1]])
        out = h.multiply_batch(sc, nmat)
        bad = [(k, pats[i][0]) for k, i in enumerate(idx) if compressed(L, as_oracle_g1(out[k])) != want[k]]
        assert not bad, bad
    finally:
        h.close()
