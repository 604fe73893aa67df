"""The checker of the zero-polynomial and recovery tests, pinned without a GPU: tests/zero_poly_model.py on the
reference's known answer (tests/golden/zero_poly_known.json, kzg-bench/src/tests/zero_poly.rs:7-50), on the reference's
test programs (zero_poly.rs, recover.rs) and on data it was sampled from; and what the library offers without a GPU:
the entry points' names and kzgamd_poly_zero_plan against the bounds the header states."""
import ctypes as C
import json
import math
import os
import random
import re

import pytest

import zero_poly_model as Z

R = Z.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kzgamd_poly_zero_partial", "kzgamd_poly_reduce_partials", "kzgamd_poly_zero_poly", "kzgamd_poly_recover",
         "kzgamd_poly_zero_info", "kzgamd_poly_zero_plan")


def _lib():
    from conftest import load_package

    return load_package("product")


def _known():
    with open(os.path.join(ROOT, "tests", "golden", "zero_poly_known.json")) as f:
        k = json.load(f)
    return k["exists"], [int(v, 16) for v in k["expected_eval"]], [int(v, 16) for v in k["expected_poly"]]


def _eval(p, x):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % R
    return acc


def _sampled(seed, n, nmissing):
    """(data, samples): the evaluations of a random polynomial of degree < n / 2, and the same with nmissing gaps"""
    rnd = random.Random(seed)
    poly = [rnd.randrange(R) for _ in range(n // 2)] + [0] * (n // 2)
    data = Z.FM.fft(poly, Z.FM.root_of_order(n))
    gone = set(rnd.sample(range(n), nmissing))
    return poly, data, [None if i in gone else v for i, v in enumerate(data)]


# ---------------------------------------------------------------- the reference's known answer and test programs
def test_zero_poly_known_and_check_test_data():
    exists, want_eval, want_poly = _known()
    missing = [i for i, e in enumerate(exists) if not e]
    assert len(missing) == 8
    ze, zp = Z.zero_poly_via_multiplication(16, 16, missing)
    assert zp == want_poly and ze == want_eval
    assert [v == 0 for v in want_eval] == [not e for e in exists]
    roots = Z.roots_of_unity(16)
    assert all(_eval(want_poly, roots[i]) == 0 for i in missing)
    assert Z.FM.ifft(want_eval, roots[1]) == want_poly
    # the long multiplication gives the same nine coefficients
    assert Z.do_zero_poly_mul_partial(16, missing, 1) == want_poly[:9]
    # and a wider table with a stride reaches the same roots
    assert Z.zero_poly_via_multiplication(64, 16, missing) == (want_eval, want_poly)


def test_reduce_partials_and_its_random_shape():
    parts = [Z.do_zero_poly_mul_partial(16, ix, 1) for ix in ([1, 3], [7, 8], [9, 10], [12, 13])]
    assert Z.reduce_partials(16, 16, parts) == Z.do_zero_poly_mul_partial(16, [1, 3, 7, 8, 9, 10, 12, 13], 1)
    rnd = random.Random(5)
    for scale, ratio in ((5, 0.3), (8, 0.5), (8, 0.7)):
        width = 1 << scale
        missing = rnd.sample(range(width), int(width * ratio))
        parts = [Z.do_zero_poly_mul_partial(width, missing[i: i + 63], 1) for i in range(0, len(missing), 63)]
        assert Z.reduce_partials(width, width, parts) == Z.do_zero_poly_mul_partial(width, missing, 1)
        assert Z.product_of_roots([Z.roots_of_unity(width)[i] for i in missing]) == Z.do_zero_poly_mul_partial(width, missing, 1)


@pytest.mark.parametrize("missing", [list(range(252)), list(range(1, 256))], ids=["zero_poly_252", "zero_poly_all_but_one"])
def test_zero_poly_252_and_all_but_one(missing):
    ze, zp = Z.zero_poly_via_multiplication(256, 256, missing)
    roots = Z.roots_of_unity(256)
    assert all(_eval(zp, roots[i]) == 0 for i in missing)
    assert [i for i, v in enumerate(ze) if v == 0] == missing
    back = Z.FM.ifft(ze, roots[1])
    assert back == zp and zp[len(missing)] == 1 and not any(zp[len(missing) + 1:])


def test_zero_poly_errors_carry_the_reference_messages():
    for args, msg in (((16, 16, list(range(16))), "Missing idxs greater than domain size"),
                      ((16, 32, [1]), "Domain size greater than fft_settings.max_width"),
                      ((16, 12, [1]), "Domain size must be a power of 2")):
        with pytest.raises(ValueError, match=msg):
            Z.zero_poly_via_multiplication(*args)
    assert Z.zero_poly_via_multiplication(16, 16, []) == ([], [])
    with pytest.raises(ValueError, match="idx array must not be empty"):
        Z.do_zero_poly_mul_partial(16, [], 1)
    with pytest.raises(ValueError, match="Expected domain size to be a power of 2"):
        Z.reduce_partials(16, 12, [[1, 1]])
    with pytest.raises(ValueError, match="partials must not be empty"):
        Z.reduce_partials(16, 16, [])
    with pytest.raises(ValueError, match="Out degree is longer"):
        Z.reduce_partials(16, 2, [[1, 1], [1, 1]])


def test_recover_simple_and_more_than_half_missing():
    poly = [0, 1, 0, 0]
    data = Z.FM.fft(poly, Z.FM.root_of_order(4))
    samples = [data[0], None, None, data[3]]
    assert Z.recover_poly_from_samples(4, samples) == data
    assert Z.recover_poly_coeffs_from_samples(4, samples) == poly
    with pytest.raises(ValueError, match="too many shards are missing"):
        Z.recover_poly_from_samples(4, [data[0], None, None, None])
    with pytest.raises(ValueError, match="too many shards are missing"):
        Z.recover_poly_from_samples(4, [None])
    with pytest.raises(ValueError, match="power of two"):
        Z.recover_poly_from_samples(4, [1, 2, 3])


@pytest.mark.parametrize("nmissing", [0, 1, 77, 128])
def test_random_recoveries_at_scale_8_give_back_the_data(nmissing):
    poly, data, samples = _sampled(40 + nmissing, 256, nmissing)
    assert Z.recover_poly_from_samples(256, samples) == data
    assert Z.recover_poly_coeffs_from_samples(256, samples) == poly
    # a wider table with a stride: the same domain
    assert Z.recover_poly_from_samples(1024, samples) == data


def test_the_shift_takes_the_exponent_i_not_i_plus_1():
    assert Z.shift_poly([1, 1, 1], 5) == [1, 5, 25]
    import poly_model as P

    assert P.unscale([1, 1, 1]) == [5, 25, 125]


# ---------------------------------------------------------------- what the library offers without a GPU
def test_header_library_and_python_mirror_name_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    pkg = _lib()
    L = pkg.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in pkg.EXPORTS and hasattr(L, name), name
    for meth in ("zero_partial", "reduce_partials", "zero_poly", "recover", "zero_plan", "zero_info"):
        assert hasattr(pkg.PolySettings, meth), meth
    for call in ("zero_partial", "reduce_partials", "zero_poly", "recover"):
        assert call in pkg.POLY_ERRORS
    assert pkg.POLY_ERRORS["recover"][2] == "Impossible to recover, too many shards are missing"
    assert pkg.POLY_ERRORS["zero_poly"][1] == "Missing idxs greater than domain size"
    # without a handle every call refuses: NULL argument, not a crash and not a CPU path
    buf = (pkg.BlstFr * 4)()
    idx = (C.c_uint64 * 4)()
    off = (C.c_size_t * 4)(0, 1, 1, 1)
    mask = (C.c_uint8 * 4)(1, 1, 1, 1)
    assert L.kzgamd_poly_zero_partial(None, buf, idx, 1, 1) == -1
    assert L.kzgamd_poly_reduce_partials(None, buf, 4, buf, off, 1) == -1
    assert L.kzgamd_poly_zero_poly(None, buf, buf, 4, idx, off, 1, 0) == -1
    assert L.kzgamd_poly_recover(None, buf, buf, mask, 4, 1, 0) == -1
    assert L.kzgamd_poly_zero_info(None, None, None) == -1


@pytest.mark.parametrize("count", [1, 63, 64, 65, 128, 129, 4095, 4096, (1 << 15) - 1])
def test_zero_plan_levels_fit_their_products_and_stay_within_the_output(count):
    plan = _lib().PolySettings.zero_plan(count)
    leaf = 64
    assert len(plan) == math.ceil(math.log2(math.ceil(count / leaf)))
    longest = 0
    entering = math.ceil(count / leaf)
    each = leaf
    for npoly, coeffs, tlen in plan:
        assert (npoly, coeffs) == (entering, each)
        assert npoly >= 2                               # a level with one polynomial would multiply nothing
        # monic split: a pair of d and e <= d low coefficients has d + e coefficients below its leading 1
        assert tlen >= 2 * coeffs and tlen & (tlen - 1) == 0
        last = count - (npoly - 1) * coeffs
        assert 1 <= last <= coeffs
        longest = max(longest, tlen)
        entering, each = (npoly + 1) // 2, 2 * coeffs
    assert entering == 1 or not plan
    assert longest <= Z.next_pow_of_2(count + 1)
    # host-only: also without a table for the levels
    assert _lib().lib().kzgamd_poly_zero_plan(count, None) == len(plan)
