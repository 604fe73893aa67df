"""The checker of kzgamd_verify_cell_kzg_proof_batch_many, pinned without a GPU (tests/vcells_many_model.py): with the
known secret the call-wide formulas (global commitment weights, one aggregated interpolation polynomial with the weights
rho^b r_b^i, the h^n factors) give exactly sum_b rho^b (P_b, L_b) of the reference's per-batch pairs; the combined
equation holds iff every batch's does for a random rho, and wrongly holds for rho = 1 on a crafted cancelling pair; the
outer challenge hashes the documented bytes; and the header, the library, the Python module and the Rust sys crate name
the three new entry points with the same parameters."""
import ctypes as C
import hashlib
import os
import random
import re

import pytest

import vcells_many_model as V

R = V.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kzgamd_verify_cell_kzg_proof_batch_many", "kzgamd_verify_cell_kzg_proof_batch_many_g1", "kzgamd_vcells_info")


def _blobs(rnd, sh, count):
    """count random polynomials of n K / 2 coefficients with their commitment scalars"""
    polys = [[rnd.randrange(R) for _ in range(sh.n * sh.K // 2)] for _ in range(count)]
    return [(p, V.evaluate(p, V.SECRET)) for p in polys]


def _opening(sh, blob, k):
    p, c = blob
    return (c, k, sh.cell(p, k), sh.proof_scalar(p, k))


def _batches(rnd, sh, blobs, sizes):
    return [[_opening(sh, rnd.choice(blobs), rnd.randrange(sh.K)) for _ in range(m)] for m in sizes]


def test_a_valid_cell_opening_satisfies_the_reference_equation():
    rnd = random.Random(1)
    for n, K in ((2, 4), (8, 8)):
        sh = V.Shape(n, K)
        blob = _blobs(rnd, sh, 1)[0]
        for k in range(K):
            c, _, values, q = _opening(sh, blob, k)
            # the interpolation polynomial of the cell is the remainder of p by X^n - h_k^n
            assert sh.interpolation(values, k) == V.long_division(blob[0], n, pow(sh.h(k), n, R))[1]
            assert V.batch_passes(sh, [(c, k, values, q)], rnd.randrange(R))
            assert not V.batch_passes(sh, [(c, k, values, (q + 1) % R)], rnd.randrange(R))


@pytest.mark.parametrize("n,K", [(4, 8), (8, 16)])
def test_call_wide_formulas_are_the_weighted_sum_of_the_batch_pairs(n, K):
    rnd = random.Random(100 + n)
    sh = V.Shape(n, K)
    blobs = _blobs(rnd, sh, 3)
    for sizes in ([1], [3, 0, 1, 5], [2, 2, 2], [0, 0], [K + 3]):
        batches = _batches(rnd, sh, blobs, sizes)
        # the same column twice in one batch and across batches, and the same tuple twice
        if len(sizes) > 1 and sizes[0] > 1:
            batches[0][1] = _opening(sh, blobs[1], batches[0][0][1])
            batches[-1][0] = batches[0][0]
        rs = [rnd.randrange(R) for _ in sizes]
        for rho in (0, 1, rnd.randrange(R)):
            want_p = want_l = 0
            for b, (cells, r) in enumerate(zip(batches, rs)):
                pb, lb = V.batch_pair(sh, cells, r)
                want_p = (want_p + pow(rho, b, R) * pb) % R
                want_l = (want_l + pow(rho, b, R) * lb) % R
            assert V.call_pair(sh, batches, rs, rho) == (want_p, want_l)
            assert V.call_passes(sh, batches, rs, rho)  # every opening is valid
    # the formulas hold for whatever the points and values carry, valid or not
    batches = _batches(rnd, sh, blobs, [2, 3])
    c, k, values, q = batches[1][2]
    batches[1][2] = ((c + 5) % R, k, [(v + 1) % R for v in values], (q + 9) % R)
    rs, rho = [rnd.randrange(R), rnd.randrange(R)], rnd.randrange(R)
    pairs = [V.batch_pair(sh, cells, r) for cells, r in zip(batches, rs)]
    assert V.call_pair(sh, batches, rs, rho) == ((pairs[0][0] + rho * pairs[1][0]) % R, (pairs[0][1] + rho * pairs[1][1]) % R)


def test_combined_equation_holds_exactly_when_every_batch_does():
    rnd = random.Random(9)
    sh = V.Shape(4, 8)
    blobs = _blobs(rnd, sh, 2)
    sizes = [3, 1, 0, 4]
    good = _batches(rnd, sh, blobs, sizes)
    rs = [rnd.randrange(R) for _ in sizes]
    assert all(V.batch_passes(sh, cells, r) for cells, r in zip(good, rs))
    assert V.call_passes(sh, good, rs, rnd.randrange(R))
    for b in (0, 1, 3):
        for at in {0, sizes[b] - 1}:
            c, k, values, q = good[b][at]
            bad_values = list(values)
            bad_values[-1] = (bad_values[-1] + 1) % R
            other = next(bl for bl in blobs if bl[1] != c)
            for broken in ((c, k, bad_values, q), (c, k, values, (q + 1) % R), (other[1], k, values, q),
                           (c, k, sh.cell(other[0], k), q)):
                bad = [list(cells) for cells in good]
                bad[b][at] = broken
                verdicts = [V.batch_passes(sh, cells, r) for cells, r in zip(bad, rs)]
                assert verdicts == [i != b for i in range(len(sizes))]
                assert not V.call_passes(sh, bad, rs, rnd.randrange(1, R))


def test_unweighted_errors_cancel_and_the_outer_weights_catch_them():
    """two batches, each with cell 0 of the same column, proofs pi + d and pi' - d: added up unweighted the d cancel"""
    rnd = random.Random(13)
    sh = V.Shape(4, 8)
    a, b = _blobs(rnd, sh, 2)
    d = rnd.randrange(1, R)
    (c0, k, v0, q0), (c1, _, v1, q1) = _opening(sh, a, 0), _opening(sh, b, 0)
    batches = [[(c0, k, v0, (q0 + d) % R)], [(c1, k, v1, (q1 - d) % R)]]
    rs = [rnd.randrange(R), rnd.randrange(R)]
    assert not V.batch_passes(sh, batches[0], rs[0]) and not V.batch_passes(sh, batches[1], rs[1])
    assert V.call_passes(sh, batches, rs, 1)
    assert not V.call_passes(sh, batches, rs, rnd.randrange(2, R))
    assert not V.call_passes(sh, batches, rs, V.outer_challenge(rs))
    # rho = 0 weighs batch 0 alone
    assert V.call_passes(sh, [[(c0, k, v0, q0)], batches[1]], rs, 0) and not V.call_passes(sh, batches, rs, 0)


def test_outer_challenge_layout():
    rs = [1, 2, R - 1]
    hand = b"KZGAMD_VCELLSET1" + bytes([0, 0, 0, 0, 0, 0, 0, 3]) + bytes(31) + b"\x01" + bytes(31) + b"\x02" + \
        bytes.fromhex("73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000000")
    assert len(hand) == 16 + 8 + 3 * 32
    assert V.outer_challenge_bytes(rs) == hand
    assert V.outer_challenge(rs) == int.from_bytes(hashlib.sha256(hand).digest(), "big") % R
    assert V.outer_challenge_bytes([]) == b"KZGAMD_VCELLSET1" + bytes(8)
    assert V.outer_challenge_bytes([R + 5]) == V.outer_challenge_bytes([5])  # canonical scalars


def test_header_library_python_module_and_rust_sys_crate_name_the_entry_points():
    from conftest import load_package
    from test_host_cpu import _c_prototypes, _rust_externs

    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    assert "KZGAMD_VCELLSET1" in hdr and "MUST be fixed after every input" in hdr
    protos = _c_prototypes()
    ext = _rust_externs(os.path.join(ROOT, "rust-kzg_amd", "rust", "src", "lib.rs"))
    pkg = load_package("product")
    L = pkg.lib()
    for name, nargs in zip(NAMES, (10, 9, 1)):
        assert len(protos[name]) == nargs, (name, protos[name])
        assert len(ext[name]) == nargs, (name, ext[name])
        assert name in pkg.EXPORTS and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    for attr in ("verify_cell_kzg_proof_batch_many", "verify_cell_kzg_proof_batch_many_g1", "vcells_info"):
        assert callable(getattr(pkg, attr)), attr
    # the slice length is host code: a small positive number, the same through both doors
    out = C.c_size_t(0)
    assert L.kzgamd_vcells_info(C.byref(out)) == 0 and L.kzgamd_vcells_info(None) == 0
    assert 1 <= out.value <= 128 and pkg.vcells_info() == out.value
    # without a settings object the GPU calls refuse: C_KZG_BADARGS, not a crash and not a CPU path
    ok = C.c_bool(True)
    num = (C.c_uint64 * 1)(0)
    pts = (pkg.BlstP1 * 2)()
    assert L.kzgamd_verify_cell_kzg_proof_batch_many(C.byref(ok), None, None, None, None, None, num, 1, None, None) == pkg.C_KZG_BADARGS
    assert L.kzgamd_verify_cell_kzg_proof_batch_many_g1(pts, None, None, None, None, num, 1, None, None) == pkg.C_KZG_BADARGS
    assert ok.value is True  # nothing written
    # the build takes the new translation unit
    import importlib.util

    spec = importlib.util.spec_from_file_location("rust_kzg_amd_build_probe", os.path.join(ROOT, "rust-kzg_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "ckzg_vcells.hip" in b.SOURCES and re.search(r"k_vcells_agg", open(os.path.join(b.CSRC, "ckzg_vcells.hip")).read())
