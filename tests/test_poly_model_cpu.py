"""The checker of the polynomial arithmetic tests, pinned without a GPU: tests/poly_model.py on the reference's own test
programs (kzg-bench/src/tests/poly.rs) and on the identities that make every result unique, and
kzgamd_poly_transform_len — host-only, reachable without a GPU — against the bounds the header states."""
import ctypes as C
import os
import random
import re

import pytest

import poly_model as P

R = P.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kzgamd_poly_new", "kzgamd_poly_free", "kzgamd_poly_info", "kzgamd_poly_eval", "kzgamd_poly_scale", "kzgamd_poly_mul",
         "kzgamd_poly_inverse", "kzgamd_poly_div", "kzgamd_poly_transform_len")

# the seven rows of test_data (poly.rs:75-122): dividend, divisor, quotient
DIV_TABLE = [
    ([-1, 0, 1], [1, 1], [-1, 1]),
    ([18, 9, -11, 12], [3, 4], [6, -5, 3]),
    ([1, 1], [-1, 0, 2], []),
    ([30, 20, 10], [10], [3, 2, 1]),
    ([0, 1, 1], [1, 1], [0, 1]),
    ([1, 1, 1], [1], [1, 1, 1]),
    ([1, 1, 1], [1, 0], [1, 1, 1]),  # the highest coefficient is zero
]


def _poly(v):
    return [c % R for c in v]


def _rand(rnd, n):
    p = [rnd.randrange(R) for _ in range(n)]
    if p and p[-1] == 0:
        p[-1] = 1
    return p


def _lib():
    from conftest import load_package

    return load_package("product")


# ---------------------------------------------------------------- the reference's test programs
def test_poly_eval_check_eval_0_check_eval_nil_check():
    assert P.evaluate([i + 1 for i in range(10)], 1) == 55
    assert P.evaluate([i + 597 for i in range(7)], 0) == 597
    assert P.evaluate([], 1) == 0


def test_poly_inverse_simple_0_and_1():
    assert P.inverse(_poly([1, -1]), 16) == [1] * 16
    assert P.inverse(_poly([1, 1]), 16) == [1 if i % 2 == 0 else R - 1 for i in range(16)]
    assert P.precision_sequence(16) == [1, 3, 7, 15] and P.precision_sequence(1) == [] and P.precision_sequence(6) == [1, 2, 5]


@pytest.mark.parametrize("row", range(6))
def test_poly_test_div_rows(row):
    a, b, q = (_poly(v) for v in DIV_TABLE[row])
    assert P.div(a, b) == q and P.long_div(a, b) == q and P.fast_div(a, b) == q


def test_poly_test_div_row_6_and_div_by_zero():
    a, b, _ = (_poly(v) for v in DIV_TABLE[6])
    for f in (P.div, P.long_div, P.fast_div):
        with pytest.raises(ValueError, match="Highest coefficient must be non-zero"):
            f(a, b)
        with pytest.raises(ValueError, match="divide by zero"):
            f(_poly([1, 1]), [])


def test_poly_mul_direct_test_and_mul_fft_test():
    a, b, want = _poly([3, 4]), _poly([6, -5, 3]), _poly([18, 9, -11, 12])
    for f in (P.mul_direct, P.mul_fft, P.mul):
        assert f(a, b, 4) == want and f(b, a, 4) == want
    assert P.mul_direct([], b, 4) == []


def test_scale_uses_the_exponent_i_plus_1():
    p = [1, 1, 7]
    inv5 = pow(5, R - 2, R)
    assert P.scale(p) == [inv5, inv5 * inv5 % R, 7 * pow(inv5, 3, R) % R]
    assert P.unscale(p) == [5, 25, 7 * 125]
    assert P.unscale(P.scale(p)) == p


# ---------------------------------------------------------------- identities on random inputs
def test_mul_direct_equals_mul_fft():
    rnd = random.Random(1)
    for la, lb, out_len in ((1, 1, 1), (5, 9, 13), (5, 9, 7), (5, 9, 40), (64, 64, 128), (70, 130, 150), (100, 3, 300)):
        a, b = _rand(rnd, la), _rand(rnd, lb)
        assert P.mul_direct(a, b, out_len) == P.mul_fft(a, b, out_len) == P.mul(a, b, out_len), (la, lb, out_len)


def test_inverse_times_b_is_one_mod_x_L():
    rnd = random.Random(2)
    for lb, L in ((1, 5), (2, 1), (2, 17), (40, 6), (40, 129), (200, 150), (70, 300)):
        b = [rnd.randrange(1, R)] + _rand(rnd, lb - 1)
        c = P.inverse(b, L)
        assert len(c) == L
        assert P.mul_direct(b, c, L) == [1] + [0] * (L - 1), (lb, L)
        assert c == P.inverse_recurrence(b, L), (lb, L)


def test_long_div_equals_fast_div_and_the_remainder_is_short():
    rnd = random.Random(3)
    for la, lb in ((2, 1), (7, 2), (10, 10), (50, 3), (300, 127), (300, 128), (300, 129), (400, 200)):
        a, b = _rand(rnd, la), _rand(rnd, lb)
        q = P.long_div(a, b)
        assert q == P.fast_div(a, b) == P.div(a, b), (la, lb)
        assert len(q) == la - lb + 1
        qb = P.mul_direct(q, b, la)
        rem = [(x - y) % R for x, y in zip(a, qb)]
        assert all(v == 0 for v in rem[lb - 1:]), (la, lb)   # deg(a - q b) < deg b = lb - 1: at most lb - 1 coefficients


# ---------------------------------------------------------------- kzgamd_poly_transform_len (host-only)
def test_header_library_and_python_mirror_name_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    pkg = _lib()
    L = pkg.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in pkg.EXPORTS and hasattr(L, name), name
    assert hasattr(pkg, "PolySettings")
    # without a handle every call refuses: NULL argument, not a crash and not a CPU path
    err = C.c_int(99)
    buf = (pkg.BlstFr * 4)()
    assert not L.kzgamd_poly_new(None, None, C.byref(err)) and err.value == -1
    assert not L.kzgamd_poly_new(None, None, None)
    L.kzgamd_poly_free(None)
    assert L.kzgamd_poly_info(None, None, None, None, None) == -1
    assert L.kzgamd_poly_eval(None, buf, buf, 1, 1, buf, 1) == -1
    assert L.kzgamd_poly_scale(None, buf, buf, 1, 1, 0) == -1
    assert L.kzgamd_poly_mul(None, buf, buf, 1, buf, 1, 1, 1, 0) == -1
    assert L.kzgamd_poly_inverse(None, buf, buf, 1, 1, 1) == -1
    assert L.kzgamd_poly_div(None, buf, buf, 1, buf, 1, 1) == -1


SIZES = [0, 1, 2, 3, 5, 17, 63, 64, 65, 127, 128, 129, 200, 1000, 4097, 16384, 32768]


def test_transform_len_of_mul_is_the_reference_length_of_the_cut_operands():
    T = _lib().PolySettings.transform_len
    for la in SIZES:
        for lb in SIZES:
            for out_len in (0, 1, 2, 64, 127, 128, 300, 40000):
                n = T("mul", la, lb, out_len)
                if la == 0 or lb == 0 or out_len == 0:
                    assert n == 0, (la, lb, out_len)      # no transform runs
                    continue
                cut = min(la, out_len) + min(lb, out_len) - 1
                assert n <= P.next_pow_of_2(cut), (la, lb, out_len)
                assert n == 0 or (n >= cut and n & (n - 1) == 0), (la, lb, out_len)
                if n == 0:
                    assert cut == 1                        # a product of two constants


def test_transform_len_of_inverse_and_div_stays_within_2L_minus_1():
    pkg = _lib()
    T = pkg.PolySettings.transform_len
    for lb in SIZES:
        for L in [v for v in SIZES if v]:
            n = T("inverse", 0, lb, L)
            assert n <= P.next_pow_of_2(2 * L - 1), (lb, L)
            assert n & (n - 1) == 0
            if lb <= 1 or L == 1:
                assert n == 0, (lb, L)                     # one inversion, no transform
            # the last Newton step multiplies c (ceil(L / 2) coefficients, twice) by b cut to L: it has to fit
            if n:
                assert n >= min(lb, L) + 2 * ((L + 1) // 2) - 2, (lb, L)
    for la in SIZES:
        for lb in SIZES:
            n = T("div", la, lb, 0)
            if lb <= 1 or la < lb:
                assert n == 0, (la, lb)                    # an error, an empty quotient, or a constant divisor
                continue
            L = la - lb + 1
            assert n <= P.next_pow_of_2(2 * L - 1), (la, lb)
            assert n >= T("inverse", 0, lb, L)
    # the reference's bench shape, 2^15 by 2^14: L = 2^14 + 1
    assert T("div", 1 << 15, 1 << 14, 0) <= 1 << 16
