"""The checker of the batched KZG check, pinned without a GPU (tests/kzg_batch_model.py): with the known secret the two
sides of the batch are [l]G and [p]G, and l == s^n p holds exactly when every tuple is valid; a single wrong value, proof
or commitment breaks it for a random weight base; the challenge hashes the buffers in the documented layout; and the
header, the library and the Python mirror name the three new entry points."""
import ctypes as C
import hashlib
import os
import random
import re

import pytest

import kzg_batch_model as B
import kzg_model as M

R = M.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kzgamd_kzg_check_batch", "kzgamd_kzg_check_batch_g1", "kzgamd_kzg_batch_challenge")


def _tuples(rnd, n, count, w):
    out = []
    for t in range(count):
        ln = rnd.choice([1, n, n + 1, 2 * n + 3])
        p = [rnd.randrange(R) for _ in range(ln)]
        x = [1, R - 1, w][t] if t < 3 else rnd.randrange(1, R)
        out.append((M.commitment_scalar(p), M.proof_scalar(p, x, n), x, M.coset_values(p, x, n, w)))
    return out


def test_interpolation_is_the_polynomial_through_the_values():
    rnd = random.Random(5)
    for n in (1, 2, 8):
        w = M.root_of_order(n)
        for x in (1, R - 1, rnd.randrange(1, R)):
            p = [rnd.randrange(R) for _ in range(3 * n + 1)]
            I = B.interpolation(M.coset_values(p, x, n, w), x, w)
            # the remainder of p by X^n - x^n is the polynomial of degree < n with p's values on the coset
            assert I == M.long_division(p, n, pow(x, n, R))[1]


@pytest.mark.parametrize("n", [1, 2, 8])
def test_batch_holds_exactly_when_every_tuple_is_valid(n):
    rnd = random.Random(40 + n)
    w = M.root_of_order(n)
    s_n = pow(M.SECRET, n, R)
    for count in (1, 2, 7):
        tuples = _tuples(rnd, n, count, w)
        assert all(B.tuple_passes(*t, n=n) for t in tuples)
        for r in (0, 1, rnd.randrange(R)):
            l, p = B.batch_scalars(tuples, n, r)
            assert l == s_n * p % R and B.batch_passes(tuples, n, r)
        # the aggregated polynomial is what the sum of the interpolation polynomials evaluates to
        r = rnd.randrange(R)
        A = B.aggregated_polynomial(tuples, n, r, w)
        want = sum(rho * M.evaluate(B.interpolation(t[3], t[2], w), M.SECRET) for rho, t in zip(B.weights(r, count), tuples)) % R
        assert len(A) == n and M.evaluate(A, M.SECRET) == want
        # one wrong value, proof or commitment, at the first and the last tuple
        for at in {0, count - 1}:
            c, q, x, ys = tuples[at]
            bad_ys = list(ys)
            bad_ys[n // 2] = (bad_ys[n // 2] + 1) % R
            for broken in ((c, q, x, bad_ys), (c, (q + 1) % R, x, ys), ((c + 1) % R, q, x, ys)):
                assert not B.tuple_passes(*broken, n=n)
                bad = tuples[:at] + [broken] + tuples[at + 1:]
                assert not B.batch_passes(bad, n, rnd.randrange(1, R))


def test_unweighted_errors_cancel_and_weights_catch_them():
    """n = 1, two openings of one polynomial with y_0 + d and y_1 - d: the sum of the two equations still holds"""
    rnd = random.Random(7)
    p = [rnd.randrange(R) for _ in range(9)]
    c, d = M.commitment_scalar(p), rnd.randrange(1, R)
    xs = [rnd.randrange(R) for _ in range(2)]
    tuples = [(c, M.proof_scalar(p, x, 1), x, [(M.evaluate(p, x) + e) % R]) for x, e in zip(xs, (d, R - d))]
    assert not B.tuple_passes(*tuples[0], n=1) and not B.tuple_passes(*tuples[1], n=1)
    assert B.batch_passes(tuples, 1, 1)
    assert not B.batch_passes(tuples, 1, rnd.randrange(2, R))
    # r = 0 weighs tuple 0 alone
    good0 = [(c, M.proof_scalar(p, xs[0], 1), xs[0], [M.evaluate(p, xs[0])]), tuples[1]]
    assert B.batch_passes(good0, 1, 0) and not B.batch_passes(tuples, 1, 0)


def test_challenge_layout():
    rnd = random.Random(11)
    n, count = 4, 3
    com, prf = rnd.randbytes(144 * count), rnd.randbytes(144 * count)
    xs, ys = rnd.randbytes(32 * count), rnd.randbytes(32 * count * n)
    hand = b"KZGAMD_CHKBATCH1" + bytes([0, 0, 0, 0, 0, 0, 0, 4]) + bytes([0, 0, 0, 0, 0, 0, 0, 3]) + com + prf + xs + ys
    assert len(hand) == 16 + 8 + 8 + count * (144 + 144 + 32 + 32 * n)
    assert B.challenge_bytes(com, prf, xs, ys, n, count) == hand
    assert B.challenge(com, prf, xs, ys, n, count) == int.from_bytes(hashlib.sha256(hand).digest(), "big") % R
    assert B.challenge_bytes(b"", b"", b"", b"", 1, 0) == b"KZGAMD_CHKBATCH1" + (1).to_bytes(8, "big") + bytes(8)


def test_header_library_and_python_mirror_name_the_batch_entry_points():
    from conftest import load_package

    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    assert "KZGAMD_CHKBATCH1" in hdr and "fixed" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    pkg = load_package("product")
    L = pkg.lib()
    for name in NAMES:
        assert name in pkg.EXPORTS and hasattr(L, name), name
    for attr in ("check_batch", "check_batch_g1"):
        assert hasattr(pkg.PolyKZGSettings, attr)
    assert "G1" in pkg.KZG_ERRORS[7]
    # the challenge is host code: it runs here, on the caller's bytes, and equals the model's
    rnd = random.Random(12)
    for n, count in ((1, 1), (8, 5), (64, 2)):
        com, prf = rnd.randbytes(144 * count), rnd.randbytes(144 * count)
        xs, ys = rnd.randbytes(32 * count), rnd.randbytes(32 * count * n)
        got = bytes(pkg.batch_challenge(com, prf, xs, ys, n, count))
        want = B.challenge(com, prf, xs, ys, n, count)
        assert int.from_bytes(got, "little") == (want << 256) % R, (n, count)  # Montgomery blst_fr
    out = pkg.BlstFr()
    assert L.kzgamd_kzg_batch_challenge(C.byref(out), None, None, None, None, 1, 0) == 0
    assert int.from_bytes(bytes(out), "little") == (B.challenge(b"", b"", b"", b"", 1, 0) << 256) % R
    pts = (pkg.BlstP1 * 2)()
    assert L.kzgamd_kzg_batch_challenge(None, pts, pts, pts, pts, 1, 1) == -1
    assert L.kzgamd_kzg_batch_challenge(C.byref(out), None, pts, pts, pts, 1, 1) == -1
    assert L.kzgamd_kzg_batch_challenge(C.byref(out), pts, pts, pts, None, 1, 1) == -1
    # without a handle the GPU calls refuse: NULL argument, not a crash and not a CPU path
    ok = C.c_bool(False)
    assert L.kzgamd_kzg_check_batch(None, C.byref(ok), None, pts, pts, pts, pts, 1, 1, None) == -1
    assert L.kzgamd_kzg_check_batch_g1(None, pts, pts, pts, pts, pts, 1, 1, None) == -1
