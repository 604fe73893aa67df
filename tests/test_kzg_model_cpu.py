"""The checker of the generic polynomial KZG tests, pinned without a GPU: the chunked quotient exactly as the kernels run
it (tests/kzg_model.py: chunked_quotient — local pass, scan with the power table, replay) equals schoolbook long division
by X^n - x^n, and both satisfy the closed forms with the known secret that the GPU tests hold the library to; and the
header, the library and the Python mirror name the six entry points."""
import ctypes as C
import os
import random
import re

import pytest

import kzg_model as M

R = M.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kzgamd_kzg_new", "kzgamd_kzg_free", "kzgamd_kzg_info", "kzgamd_kzg_commit", "kzgamd_kzg_open", "kzgamd_kzg_check")


def _lengths(n):
    edge = {n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1}
    return sorted(v for v in set(range(1, 131)) | edge if v >= 1)


@pytest.mark.parametrize("chunk", [1, 3, 16])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_chunked_model_equals_long_division_and_closed_forms(n, chunk):
    rnd = random.Random(100 * n + chunk)
    w = M.root_of_order(n)
    s = M.SECRET
    for ln in _lengths(n):
        p = [rnd.randrange(R) for _ in range(ln)]
        for x in (0, 1, R - 1, rnd.randrange(R)):
            c = pow(x, n, R)
            q, r = M.long_division(p, n, c)
            assert len(q) == max(ln - n, 0) and len(r) == n
            # wave 64 as the kernels; wave 4 takes the path across waves at these lengths too
            for wave in (64, 4):
                assert M.chunked_quotient(p, n, c, chunk, wave) == (q, r), (ln, n, chunk, x, wave)
            # p = q (X^n - c) + r at the secret, and the proof scalar the GPU tests use
            ps, qs, rs = M.evaluate(p, s), M.evaluate(q, s), M.evaluate(r, s)
            assert ps == (qs * (pow(s, n, R) - c) + rs) % R
            assert M.proof_scalar(p, x, n) == qs
            assert M.commitment_scalar(p) == ps
            # the values on the coset are the remainder's: forward transform of r_j x^j
            ys = M.coset_values(p, x, n, w)
            assert ys == [M.evaluate(r, x * pow(w, i, R) % R) for i in range(n)]
            assert ys == [sum(r[j] * pow(x, j, R) * pow(w, i * j, R) for j in range(n)) % R for i in range(n)]


def test_header_library_and_python_mirror_name_the_six_entry_points():
    from conftest import load_package

    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    pkg = load_package("product")
    L = pkg.lib()
    for name in NAMES:
        assert name in pkg.EXPORTS and hasattr(L, name), name
    assert hasattr(pkg, "PolyKZGSettings") and pkg.KZG_ERRORS[1] == "Polynomial is longer than secret g1"
    # without handles every call refuses: NULL argument, not a crash and not a CPU path
    err = C.c_int(99)
    pts = (pkg.BlstP1 * 4)()
    assert not L.kzgamd_kzg_new(None, pts, 4, None, 0, None, C.byref(err)) and err.value == -1
    assert not L.kzgamd_kzg_new(None, pts, 0, None, 0, None, C.byref(err)) and err.value == 1
    assert not L.kzgamd_kzg_new(None, pts, 4, None, 0, None, None)  # err may be NULL
    L.kzgamd_kzg_free(None)
    assert L.kzgamd_kzg_info(None, None, None, None, None) == -1
    assert L.kzgamd_kzg_commit(None, pts, pts, 1, 1) == -1
    assert L.kzgamd_kzg_open(None, pts, None, pts, 1, 1, pts, 1, 1) == -1
    assert L.kzgamd_kzg_check(None, None, pts, pts, pts, pts, 1, 1) == -1
