"""The checker of the generic FK20 tests, pinned without a GPU: the reference's algorithm restated on integers
(tests/fk20_model.py: fk20_restated) equals the closed form the GPU tests hold the library to (fk20_closed_form) at
every position, for the shapes of the reference's own tests and the EIP-7594 cell shape; and the C ABI refuses to
build a handle without an NTT handle, which is what a machine without a device has (the product has no CPU fallback)."""
import ctypes as C
import random

import pytest

import fk20_model as M


@pytest.mark.parametrize("n,l", [(16, 1), (256, 1), (512, 1), (16, 16), (64, 32), (256, 16), (512, 16), (4096, 64)])
def test_restated_algorithm_equals_closed_form(n, l):
    rnd = random.Random(n * 131 + l)
    w = M.root_of_order(2 * n // l)
    polys = [[rnd.randrange(M.R) for _ in range(n)]]
    if n == 16:
        polys.append(M.fk_single_poly())
    polys.append(M.fk_multi_poly(n, l))
    for p in polys:
        assert M.fk20_restated(p, l, M.SECRET, w) == M.fk20_closed_form(p, l, M.SECRET, w)


def test_toeplitz_coefficients_have_the_reference_shape():
    p = list(range(1, 33))
    # k = 8, k2 = 16: head, k + 1 zeros, then every 4th coefficient from 2 l - offset - 1
    assert M.toeplitz_coeffs_stride(p, 1, 4) == [p[30]] + [0] * 9 + [p[6], p[10], p[14], p[18], p[22], p[26]]
    # k <= 2: nothing but the head
    assert M.toeplitz_coeffs_stride(p, 0, 32) == [p[31], 0]
    assert M.toeplitz_coeffs_stride(p, 3, 16) == [p[28], 0, 0, 0]


def test_fk20_new_without_an_ntt_handle_is_refused():
    """no GPU: kzgamd_ntt_new returns NULL, and kzgamd_fk20_new over it NULL with a negative *err"""
    from conftest import load_package

    pkg = load_package("product")
    L = pkg.lib()
    for name in ("kzgamd_fk20_new", "kzgamd_fk20_free", "kzgamd_fk20_da", "kzgamd_fk20_info"):
        assert hasattr(L, name) and name in pkg.EXPORTS
    pts = (pkg.BlstP1 * 16)()
    err = C.c_int(99)
    assert not L.kzgamd_fk20_new(None, pts, 16, 32, 1, None, C.byref(err))
    assert err.value < 0
    assert not L.kzgamd_fk20_new(None, pts, 16, 32, 1, None, None)  # err may be NULL
    L.kzgamd_fk20_free(None)
    out = (pkg.BlstP1 * 32)()
    assert L.kzgamd_fk20_da(None, out, pts, 16, 1, 0) == -1
    assert L.kzgamd_fk20_info(None, None, None, None) == -1
    if pkg.device_count() < 1:
        with pytest.raises(pkg.KzgAmdError):
            pkg.FFTSettings(5)
