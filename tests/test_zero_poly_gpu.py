"""Zero polynomials and sample recovery on the GPU (kzgamd_poly_zero_partial, _reduce_partials, _zero_poly, _recover).

Every output is a field element with one value — a monic product of linear factors, its transform, a pointwise quotient
whose divisor is never zero — so every comparison is exact.  The anchor is tests/zero_poly_model.py (the reference's
zero_poly.rs and recovery.rs on Python integers, pinned on the CPU by tests/test_zero_poly_model_cpu.py on the
reference's known answer); recoveries are also anchored by construction, on the data the samples were taken from.

Sizes sit on the boundaries the kernels have: the 64 roots of a leaf wave, one pair, a level with an odd polynomial, a
last polynomial shorter than its neighbours, a product that fills its domain, the 4096-point tile of the transform, and
the direct-to-tree switch zero_info() reports."""
import ctypes as C
import json
import os
import random
import threading

import pytest

import zero_poly_model as Z

pytestmark = pytest.mark.gpu
R = Z.R
MB = 1 << 20
RINV = pow(1 << 256, R - 2, R)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fr(vals):
    raw = b"".join(((v << 256) % R).to_bytes(32, "little") for v in vals)
    arr = (C.c_uint64 * (4 * max(1, len(vals))))()
    C.memmove(arr, raw, len(raw))
    return arr


def _ints(arr, count):
    raw = bytes(arr)
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") * RINV % R for i in range(count)]


_cache = {}


def _once(key, make):
    """references are computed once and shared by the two library flavours"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _model_zero(width, n, missing):
    def make():
        return Z.zero_poly_via_multiplication(width, n, missing) if missing else Z.empty_product(n)
    return _once(("zero", width, n, tuple(missing)), make)


def _check_zero(ps, width, n, lists, forms=(0, 1, 2)):
    """every form of one call against the model, problem by problem"""
    want_e = [v for m in lists for v in _model_zero(width, n, m)[0]]
    want_p = [v for m in lists for v in _model_zero(width, n, m)[1]]
    for form in forms:
        ze, zp = ps.zero_poly(n, lists, form=form)
        assert _ints(zp, len(lists) * n) == want_p, (n, [len(m) for m in lists], form)
        assert _ints(ze, len(lists) * n) == want_e, (n, [len(m) for m in lists], form)


def _garbage(nbytes):
    buf = (C.c_uint8 * nbytes)()
    C.memset(buf, 0xA5, nbytes)
    return buf


def _untouched(buf):
    return bytes(buf) == b"\xa5" * len(buf)


# ---------------------------------------------------------------- zero_poly
def test_zero_poly_across_the_leaf_and_level_boundaries(kzg):
    """domain 256: one wave, a full wave, one pair, an odd level, a short last polynomial, a product filling the domain"""
    rnd = random.Random(31)
    fs = kzg.FFTSettings(8)
    try:
        with kzg.PolySettings(fs) as ps:
            leaf, direct_max = ps.zero_info()
            assert leaf == 64 and direct_max >= 0
            for count in (1, 63, 64, 65, 127, 128, 129, 192, 193):
                missing = _once(("m256", count), lambda: rnd.sample(range(256), count))
                _check_zero(ps, 256, 256, [missing])
            _check_zero(ps, 256, 256, [list(range(252))])       # zero_poly_252
            _check_zero(ps, 256, 256, [list(range(1, 256))])    # zero_poly_all_but_one: 256 coefficients, the last is 1
    finally:
        fs.close()


def test_zero_poly_known_answer(kzg):
    with open(os.path.join(ROOT, "tests", "golden", "zero_poly_known.json")) as f:
        k = json.load(f)
    missing = [i for i, e in enumerate(k["exists"]) if not e]
    fs = kzg.FFTSettings(4)
    try:
        with kzg.PolySettings(fs) as ps:
            for form in (0, 1, 2):
                ze, zp = ps.zero_poly(16, [missing], form=form)
                assert _ints(ze, 16) == [int(v, 16) for v in k["expected_eval"]], form
                assert _ints(zp, 16) == [int(v, 16) for v in k["expected_poly"]], form
    finally:
        fs.close()


@pytest.mark.parametrize("scale,count", [(13, 4097), (15, 2049)], ids=["4097-of-8192", "2049-of-8192-stride-4"])
def test_zero_poly_products_beyond_one_transform_tile(kzg, scale, count):
    """the last products are longer than the 4096-point single-tile transform"""
    missing = _once(("m8192", count), lambda: random.Random(32 + count).sample(range(8192), count))
    fs = kzg.FFTSettings(scale)
    try:
        with kzg.PolySettings(fs) as ps:
            _check_zero(ps, 1 << scale, 8192, [missing], forms=(1, 2))
    finally:
        fs.close()


def test_zero_poly_unequal_problems_in_one_call_and_repeated_indices(kzg):
    rnd = random.Random(33)
    lists = _once("m1024", lambda: [rnd.sample(range(1024), c) for c in (0, 1, 64, 300, 1023)])
    fs = kzg.FFTSettings(10)
    try:
        with kzg.PolySettings(fs) as ps:
            _check_zero(ps, 1024, 1024, lists)
            ze, zp = ps.zero_poly(1024, lists[:1])
            assert _ints(zp, 1024) == [1] + [0] * 1023 and _ints(ze, 1024) == [1] * 1024   # the empty product
            # a repeated index is a repeated root
            rep = [5, 7, 5, 5, 900] + list(range(100, 170))
            _check_zero(ps, 1024, 1024, [rep, [3, 3]])
            # one output alone
            want_e, want_p = _model_zero(1024, 1024, lists[3])
            for form in (1, 2):
                ze, zp = ps.zero_poly(1024, [lists[3]], form=form, want_poly=False)
                assert zp is None and _ints(ze, 1024) == want_e
                ze, zp = ps.zero_poly(1024, [lists[3]], form=form, want_eval=False)
                assert ze is None and _ints(zp, 1024) == want_p
    finally:
        fs.close()


def test_zero_poly_error_codes_write_nothing(kzg):
    L = kzg.lib()
    fs = kzg.FFTSettings(4)
    try:
        with kzg.PolySettings(fs) as ps:
            def call(n, lists, form=0):
                flat = [i for m in lists for i in m]
                offs = [0]
                for m in lists:
                    offs.append(offs[-1] + len(m))
                ze, zp = _garbage(32 * 64), _garbage(32 * 64)
                rc = L.kzgamd_poly_zero_poly(ps.handle, ze, zp, n, (C.c_uint64 * max(1, len(flat)))(*flat),
                                             (C.c_size_t * len(offs))(*offs), len(lists), form)
                return rc, _untouched(ze) and _untouched(zp)

            assert call(16, [[1], list(range(16))]) == (1, True)
            assert call(0, [[]]) == (1, True)          # an empty list has >= 0 entries: the first check comes first
            assert call(32, [[1]]) == (2, True)
            assert call(12, [[1]]) == (3, True)
            assert call(16, [[1], [2, 16]]) == (5, True)
            assert call(16, [[1]], form=3) == (-1, True)
            assert call(16, []) == (0, True)           # no problem: ok, nothing written
            for what, code in (("zero_poly", 1), ("zero_poly", 2), ("zero_poly", 3)):
                assert kzg.POLY_ERRORS[what][code]
            with pytest.raises(kzg.KzgAmdError, match="Missing idxs greater than domain size") as e:
                ps.zero_poly(16, [list(range(16))])
            assert e.value.code == 1
    finally:
        fs.close()


# ---------------------------------------------------------------- zero_partial / reduce_partials
def test_reduce_partials_the_reference_shapes(kzg):
    fs = kzg.FFTSettings(4)
    try:
        with kzg.PolySettings(fs) as ps:
            groups = ([1, 3], [7, 8], [9, 10], [12, 13])
            parts = [_ints(ps.zero_partial(ix, 1), 3) for ix in groups]
            assert parts == [Z.do_zero_poly_mul_partial(16, ix, 1) for ix in groups]
            got = _ints(ps.reduce_partials(16, _fr([c for p in parts for c in p]), [3] * 4), 9)
            assert got == Z.do_zero_poly_mul_partial(16, [i for ix in groups for i in ix], 1)
            assert got == _ints(ps.zero_partial([i for ix in groups for i in ix], 1), 9)
    finally:
        fs.close()
    rnd = random.Random(34)
    fs = kzg.FFTSettings(8)
    try:
        with kzg.PolySettings(fs) as ps:
            missing = _once("rp256", lambda: rnd.sample(range(256), 179))
            chunks = [missing[i: i + 63] for i in range(0, 179, 63)]
            parts = [_ints(ps.zero_partial(ix, 1), len(ix) + 1) for ix in chunks]
            assert parts == _once("rp256p", lambda: [Z.do_zero_poly_mul_partial(256, ix, 1) for ix in chunks])
            want = _once("rp256w", lambda: Z.do_zero_poly_mul_partial(256, missing, 1))
            assert _ints(ps.reduce_partials(256, _fr([c for p in parts for c in p]), [len(p) for p in parts]), 180) == want
            assert _ints(ps.zero_partial(missing, 1), 180) == want
            # not monic, and constants among them: any polynomials multiply
            polys = _once("rpany", lambda: [[rnd.randrange(R) for _ in range(n)] for n in (1, 40, 1, 7, 100)])
            prod = _once("rpanyw", lambda: Z.reduce_partials(256, 256, polys))
            assert _ints(ps.reduce_partials(256, _fr([c for p in polys for c in p]), [len(p) for p in polys]), 145) == prod
    finally:
        fs.close()


def test_zero_partial_of_1000_roots_with_a_stride(kzg):
    idxs = _once("zp1000", lambda: [random.Random(35).randrange(1024) for _ in range(1000)])   # with repeats
    fs = kzg.FFTSettings(12)
    try:
        with kzg.PolySettings(fs) as ps:
            roots = Z.roots_of_unity(4096)
            want = _once("zp1000w", lambda: Z.product_of_roots([roots[4 * i] for i in idxs]))
            assert _ints(ps.zero_partial(idxs, 4), 1001) == want
            assert _ints(ps.zero_partial([1024], 4), 2) == [R - 1, 1]      # roots[max_width] is the last entry of the table
    finally:
        fs.close()


def test_zero_partial_and_reduce_partials_error_codes_write_nothing(kzg):
    L = kzg.lib()
    fs = kzg.FFTSettings(4)
    try:
        with kzg.PolySettings(fs) as ps:
            def partial(idxs, stride):
                out = _garbage(32 * 80)
                rc = L.kzgamd_poly_zero_partial(ps.handle, out, (C.c_uint64 * max(1, len(idxs)))(*idxs), len(idxs), stride)
                return rc, _untouched(out)

            assert partial([], 1) == (1, True)
            assert partial([3, 17], 1) == (2, True)
            assert partial([3, 9], 2) == (2, True)
            assert partial([1 << 63], 4) == (2, True)              # the product does not wrap round
            assert partial(list(range(16)) * 4 + [1], 1) == (4, True)   # 65 roots: a transform of 128 on a width of 16
            assert partial([16], 1) == (0, False)

            def reduce(domain, lens):
                out = _garbage(32 * 80)
                parts = _fr([1] * max(1, sum(lens)))
                rc = L.kzgamd_poly_reduce_partials(ps.handle, out, domain, parts, (C.c_size_t * max(1, len(lens)))(*lens), len(lens))
                return rc, _untouched(out)

            assert reduce(12, [2, 2]) == (1, True)
            assert reduce(0, [2, 2]) == (1, True)
            assert reduce(16, []) == (2, True)
            assert reduce(16, [2, 0, 2]) == (5, True)
            assert reduce(8, [5, 5]) == (3, True)
            assert reduce(32, [5, 5]) == (4, True)
            assert reduce(16, [9, 8]) == (0, False)                # 16 coefficients fill the domain
            with pytest.raises(kzg.KzgAmdError, match="idx array must not be empty"):
                ps.zero_partial([], 1)
            with pytest.raises(kzg.KzgAmdError, match="partials must not be empty"):
                ps.reduce_partials(16, _fr([1]), [])
    finally:
        fs.close()


# ---------------------------------------------------------------- recover
def _sampled(seed, n, nmissing):
    """(poly, data, values, present): data = the evaluations of a random polynomial of degree < n / 2; values = data with
    garbage in the nmissing gaps that present marks"""
    def make():
        rnd = random.Random(seed)
        poly = [rnd.randrange(R) for _ in range(n // 2)] + [0] * (n // 2)
        data = Z.FM.fft(poly, Z.FM.root_of_order(n))
        gone = set(rnd.sample(range(n), nmissing))
        values = [rnd.randrange(R) if i in gone else v for i, v in enumerate(data)]
        return poly, data, values, bytes(0 if i in gone else 1 for i in range(n))
    return _once(("sampled", seed, n, nmissing), make)


def test_recover_simple(kzg):
    fs = kzg.FFTSettings(2)
    try:
        with kzg.PolySettings(fs) as ps:
            poly = [0, 1, 0, 0]
            data = Z.FM.fft(poly, Z.FM.root_of_order(4))
            values = _fr([data[0], 12345, 67890, data[3]])
            assert _ints(ps.recover(values, bytes([1, 0, 0, 1]), 4), 4) == data
            assert _ints(ps.recover(values, bytes([1, 0, 0, 1]), 4, coeffs=True), 4) == poly
            with pytest.raises(kzg.KzgAmdError, match="too many shards are missing") as e:   # more_than_half_missing
                ps.recover(values, bytes([1, 0, 0, 0]), 4)
            assert e.value.code == 2
            with pytest.raises(kzg.KzgAmdError, match="too many shards are missing"):
                ps.recover(values, bytes([0]), 1)
            assert _ints(ps.recover(_fr([77]), bytes([1]), 1), 1) == [77]
    finally:
        fs.close()


def test_recover_at_the_half_missing_limit_and_without_gaps(kzg):
    fs = kzg.FFTSettings(8)
    L = kzg.lib()
    try:
        with kzg.PolySettings(fs) as ps:
            for nmissing in (128, 1, 0):
                poly, data, values, present = _sampled(50, 256, nmissing)
                assert _ints(ps.recover(_fr(values), present, 256), 256) == data, nmissing
                assert _ints(ps.recover(_fr(values), present, 256, coeffs=True), 256) == poly, nmissing
                samples = [v if p else None for v, p in zip(values, present)]
                assert Z.recover_poly_from_samples(256, samples) == data
            poly, data, values, present = _sampled(51, 256, 129)
            out = _garbage(32 * 256)
            mask = (C.c_uint8 * 256).from_buffer_copy(present)
            assert L.kzgamd_poly_recover(ps.handle, out, _fr(values), mask, 256, 1, 0) == 2 and _untouched(out)
            assert L.kzgamd_poly_recover(ps.handle, out, _fr(values), mask, 12, 1, 0) == 1 and _untouched(out)
            assert L.kzgamd_poly_recover(ps.handle, out, _fr(values), mask, 0, 1, 0) == 1 and _untouched(out)
            ok = (C.c_uint8 * 512)(*([1] * 512))
            assert L.kzgamd_poly_recover(ps.handle, out, _fr(values * 2), ok, 512, 1, 0) == 3 and _untouched(out)
            assert L.kzgamd_poly_recover(ps.handle, out, _fr(values), mask, 256, 0, 0) == 0 and _untouched(out)
    finally:
        fs.close()


@pytest.mark.parametrize("coeffs", [False, True], ids=["evaluations", "coefficients"])
def test_recover_8192_with_half_missing(kzg, coeffs):
    poly, data, values, present = _sampled(52, 8192, 4096)
    fs = kzg.FFTSettings(13)
    try:
        with kzg.PolySettings(fs) as ps:
            assert _ints(ps.recover(_fr(values), present, 8192, coeffs=coeffs), 8192) == (poly if coeffs else data)
    finally:
        fs.close()


def test_recover_is_a_function_of_the_input_alone(kzg):
    """samples no polynomial of degree < n / 2 fits, a present sample that is 0, garbage in the gaps"""
    n = 1024

    def make():
        rnd = random.Random(53)
        gone = set(rnd.sample(range(n), 400))
        samples = [None if i in gone else rnd.randrange(R) for i in range(n)]
        samples[next(i for i in range(n) if i not in gone)] = 0
        return samples, Z.recover_poly_coeffs_from_samples(n, samples), Z.recover_poly_from_samples(n, samples)
    samples, want_c, want_e = _once("anydata", make)
    present = bytes(0 if s is None else 1 for s in samples)
    rnd = random.Random(54)
    fs = kzg.FFTSettings(10)
    try:
        with kzg.PolySettings(fs) as ps:
            one = [rnd.randrange(R) if s is None else s for s in samples]
            two = [R - 1 if s is None else s for s in samples]
            got = [bytes(ps.recover(_fr(v), present, n, coeffs=True)) for v in (one, two)]
            assert got[0] == got[1]
            assert _ints(got[0], n) == want_c
            assert _ints(ps.recover(_fr(one), present, n), n) == want_e
    finally:
        fs.close()


def test_recover_a_batch_with_unequal_gaps(kzg):
    n = 512
    sets = [_sampled(60 + k, n, m) for k, m in enumerate((0, 1, 200, 256))]
    fs = kzg.FFTSettings(9)
    try:
        with kzg.PolySettings(fs) as ps:
            values = _fr([v for s in sets for v in s[2]])
            present = b"".join(s[3] for s in sets)
            assert _ints(ps.recover(values, present, n, nprob=4), 4 * n) == [v for s in sets for v in s[1]]
            assert _ints(ps.recover(values, present, n, nprob=4, coeffs=True), 4 * n) == [v for s in sets for v in s[0]]
    finally:
        fs.close()


# ---------------------------------------------------------------- threads and lifecycle
def test_threads_share_a_handle_and_free_returns_hbm(kzg):
    import torch

    import poly_model as P

    n = 512
    sets = [_sampled(70 + k, n, 256 - 3 * k) for k in range(2)]
    rnd = random.Random(71)
    A, B = [rnd.randrange(R) for _ in range(200)], [rnd.randrange(R) for _ in range(150)]
    want_mul = _once("thrmul", lambda: P.mul_direct(A, B, 349))
    fs = kzg.FFTSettings(9)
    try:
        with kzg.PolySettings(fs) as ps:
            failures = []

            def recover(t):
                try:
                    _, data, values, present = sets[t]
                    v = _fr(values)
                    for _ in range(4):
                        assert _ints(ps.recover(v, present, n), n) == data
                except Exception as e:  # noqa: BLE001
                    failures.append((t, repr(e)))

            def multiply(t):
                try:
                    fa, fb = _fr(A), _fr(B)
                    for _ in range(4):
                        assert _ints(ps.mul(fa, 200, fb, 150, 349, 1, 2), 349) == want_mul
                except Exception as e:  # noqa: BLE001
                    failures.append((t, repr(e)))

            ts = [threading.Thread(target=recover, args=(0,)), threading.Thread(target=recover, args=(1,)),
                  threading.Thread(target=multiply, args=(2,))]
            for th in ts:
                th.start()
            for th in ts:
                th.join()
            assert failures == []

        _, data, values, present = sets[0]
        missing = [i for i in range(n) if not present[i]]

        def cycle():
            with kzg.PolySettings(fs) as ps:
                return (bytes(ps.recover(_fr(values), present, n)), bytes(ps.zero_poly(n, [missing], form=2)[1]),
                        bytes(ps.zero_partial(missing, 1)))

        want = cycle()
        assert _ints(want[0], n) == data
        torch.cuda.synchronize()
        base, _ = torch.cuda.mem_get_info(0)
        deltas = []
        for _ in range(5):
            assert cycle() == want
            torch.cuda.synchronize()
            free, _ = torch.cuda.mem_get_info(0)
            deltas.append((base - free) / MB)
            assert base - free <= 8 * MB, deltas
        print("zero poly lifecycle: HBM delta MB per cycle:", ["%.2f" % d for d in deltas])
    finally:
        fs.close()
