"""The wide table in the limbs of the accumulation chain (g1s::WidePt30: x and y as 13 x 30-bit limbs, the infinity flag
at word 26) and psi in the constants of the way back (g1s::to_xyzz28 with a part), against the oracle's naive MSM, byte
for byte.  The shapes are those of test_fbw_accum_fp30s_gpu.py; the 4096-point suites drive every instantiation, the
quad kernel and infinite bases through the public entry points.  Here: what the new layout can break, at the smallest
size.

n = 64 generated bases, a 0.25 GB table budget.  Bases 8..11 are one point, base 5 is at infinity (every slot of its
rows carries the flag in its new place), base 2 is the generator.
Forms: the GLV table (`glv`), the one without the split (`plain`, fbw_glv=0), and a segmented handle (4 rows of 64
bases) with the tuning key `spl` at 8 and 16.  Batches of 3 and 256 MSMs; the segmented handle takes whole matrices,
so 4 (one matrix) and 256.
Scalars: 0, 1, r - 1; every window at digit 1 and at 2^(c-1) (the first and the last slot of a table row), and at
2^(c-1) + 1 (a negative digit and a carry in every window), each in the k1 half and in the k2 half, and over the whole
width for the form without the split; random scalars with only a k2 half (every finite partial sum of the odd lanes
goes back through the constant for beta and the negated Y, every even lane is empty), with only a k1 half; three random
sets."""
import ctypes as C
import random

import pytest

import oracle_ffi as O
from test_msm_gpu import as_oracle_g1, compressed, gen_points

pytestmark = pytest.mark.gpu

N = 64
X2 = 0xD201000000010000 ** 2  # k = k1 + k2 * X2 (glv.hip.h)
INFINITE, GENERATOR = 5, 2


def window_patterns(c, bits):
    nw = bits // c
    half = 1 << (c - 1)
    return [("digit1", sum(1 << (c * w) for w in range(nw))),
            ("half", sum(half << (c * w) for w in range(nw))),
            ("half_plus1", sum((half + 1) << (c * w) for w in range(nw)))]


def patterns(c, seed):
    """[(name, 64 scalars)]"""
    rnd = random.Random(seed)
    pats = [("zero_one_rminus1", [(0, 1, O.R - 1)[i % 3] for i in range(N)])]
    for name, v in window_patterns(c, 126):       # the GLV split leaves a 126-bit value whole in one half
        pats.append((name + "_k1", [v] * N))
        pats.append((name + "_k2", [v * X2 % O.R] * N))
    for name, v in window_patterns(c, 254):       # the windows of the form without the split
        assert v < O.R
        pats.append((name + "_full", [v] * N))
    pats.append(("only_k2", [rnd.randrange(1, 1 << 126) * X2 % O.R for _ in range(N)]))
    pats.append(("only_k1", [rnd.randrange(1, 1 << 126) for _ in range(N)]))
    for k in range(3):
        pats.append(("random%d" % k, [rnd.randrange(O.R) for _ in range(N)]))
    return pats


_cache = {}


def bases(L, seed):
    if seed in _cache:
        return _cache[seed]
    pts = gen_points(L, N, random.Random(seed))
    for i in (9, 10, 11):
        pts[i] = pts[8]
    pts[INFINITE] = O.G1Affine()
    g = O.G1()
    L.og1_generator(C.byref(g))
    L.og1_to_affine(C.byref(pts[GENERATOR]), C.byref(g))
    _cache[seed] = pts
    return pts


def reference(L, seed, c):
    """(bases, patterns, expected commitments) — computed once per base set and window width, shared, never changed"""
    if (seed, c) not in _cache:
        pts = bases(L, seed)
        pats = patterns(c, seed + 1000)
        want = []
        for _, v in pats:
            e = O.G1()
            L.omsm_naive(C.byref(e), pts, O.fr_array(v), N)
            want.append(compressed(L, e))
        assert len(set(want)) > len(want) - 3
        _cache[(seed, c)] = (pts, pats, want)
    return _cache[(seed, c)]


@pytest.mark.parametrize("form", ["glv", "plain"])
def test_prepared_batches_against_the_oracle(oracle, kzg, form):
    L = oracle.lib()
    pts = bases(L, 0x530)
    h = kzg.prepare_multi_scalar_mult(pts, N, kzg.make_config(table_budget_gb=0.25, tuning={"fbw_glv": 0} if form == "plain" else {}))
    try:
        info = h.info()
        assert info["wide_table"] and info["wide_glv"] == (form == "glv"), info
        pts, pats, want = reference(L, 0x530, info["window_bits"])
        for nbatch in (3, 256):
            for first in range(0, len(pats), nbatch):
                idx = [(first + j) % len(pats) for j in range(nbatch)]
                sc = O.fr_array([s for i in idx for s in pats[i][1]])
                got = kzg.multi_scalar_mult_prepared_batch(h, sc, N, nbatch)
                bad = [pats[i][0] for b, i in enumerate(idx) if compressed(L, as_oracle_g1(got[b])) != want[i]]
                assert not bad, (nbatch, bad)
    finally:
        h.close()


@pytest.mark.parametrize("spl", [8, 16])
def test_a_segmented_handle_against_the_oracle(oracle, kzg, spl):
    L = oracle.lib()
    rows = 4
    per_row = [bases(L, 0x540 + r) for r in range(rows)]
    flat = (O.G1Affine * (rows * N))(*[p for r in per_row for p in r[:N]])
    h = kzg.MatrixMsm(flat, rows, N, kzg.make_config(table_budget_gb=0.25, tuning={"spl": spl}))
    try:
        info = h.info()
        assert info["wide_table"] and info["wide_glv"], info
        refs = [reference(L, 0x540 + r, info["window_bits"]) for r in range(rows)]
        npat = len(refs[0][1])
        for nmat in (1, 256 // rows):
            for first in range(0, npat, nmat * rows):
                idx = [(first + k) % npat for k in range(nmat * rows)]  # MSM k runs over the bases of row k % rows
                sc = O.fr_array([s for k, i in enumerate(idx) for s in refs[k % rows][1][i][1]])
                out = h.multiply_batch(sc, nmat)
                bad = [(k, refs[k % rows][1][i][0]) for k, i in enumerate(idx)
                       if compressed(L, as_oracle_g1(out[k])) != refs[k % rows][2][i]]
                assert not bad, (nmat, bad)
    finally:
        h.close()
