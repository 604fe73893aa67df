"""Batched polynomial arithmetic on the GPU (kzgamd_poly_*): eval, scale / unscale, mul in its three forms, inverse, div.

Every result is a field element with one value, so every comparison is exact.  Anchors, none of them the code under test:
tests/poly_model.py (the reference's poly.rs on Python integers, pinned on the CPU by tests/test_poly_model_cpu.py) and
algebraic identities in Python integers.  Large quotients are anchored by construction: a = q b + r with random q, b and
r shorter than b, formed with the model's transform product; the call must return exactly q.

Sizes sit on the boundaries the kernels have: the chunk and the wave of the scan, the 4096-point tile of the NTT, the
reference's 64 / 128 thresholds, and the direct-to-transform switches info() reports."""
import ctypes as C
import random
import threading

import pytest

import poly_model as P

pytestmark = pytest.mark.gpu
R = P.R
MB = 1 << 20
RINV = pow(1 << 256, R - 2, R)


def _fr(vals):
    raw = b"".join(((v << 256) % R).to_bytes(32, "little") for v in vals)
    arr = (C.c_uint64 * (4 * max(1, len(vals))))()
    C.memmove(arr, raw, len(raw))
    return arr


def _ints(arr, count):
    raw = bytes(arr)
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") * RINV % R for i in range(count)]


def _rand(rnd, n):
    p = [rnd.randrange(R) for _ in range(n)]
    if p and p[-1] == 0:
        p[-1] = 1
    return p


def _flat(polys):
    return _fr([c for p in polys for c in p])


def _fit(p, n):
    """the first n coefficients of p, zero-extended"""
    return (list(p) + [0] * n)[:n]


_cache = {}


def _once(key, make):
    """references are computed once and shared by the two library flavours"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _by_construction(seed, la, lb):
    """(a, b, q) with a = q b + r, len(q) = la - lb + 1, len(r) < lb"""
    def make():
        rnd = random.Random(seed)
        q, b = _rand(rnd, la - lb + 1), _rand(rnd, lb)
        r = [rnd.randrange(R) for _ in range(lb - 1)]
        qb = P.mul_fft(q, b, la) if min(len(q), lb) > 32 else P.mul_direct(q, b, la)
        return [(x + y) % R for x, y in zip(qb, _fit(r, la))], b, q
    return _once(("div", seed, la, lb), make)


# ---------------------------------------------------------------- eval
def test_eval_across_chunk_and_wave_boundaries(kzg):
    rnd = random.Random(11)
    fs = kzg.FFTSettings(4)
    try:
        with kzg.PolySettings(fs) as ps:
            width, chunk, mul_max, inv_max = ps.info()
            assert width == 16 and chunk >= 1 and mul_max >= 1 and inv_max >= 1
            xs = [0, 1, R - 1, rnd.randrange(R)]
            lens = [0, 1, 2, chunk - 1, chunk, chunk + 1, 64 * chunk - 1, 64 * chunk + 1, 3 * 64 * chunk + 5]
            for ln in sorted(set(v for v in lens if v >= 0)):
                polys = [[rnd.randrange(R) for _ in range(ln)] for _ in range(3)]
                got = _ints(ps.eval(_flat(polys), ln, 3, _fr(xs), 4), 12)
                assert got == [P.evaluate(p, x) for p in polys for x in xs], ln
    finally:
        fs.close()


def test_eval_longer_than_a_block_of_wave_summaries(kzg):
    """more than 64 waves of chunks: the carry kernel takes two blocks of summaries"""
    rnd = random.Random(12)
    fs = kzg.FFTSettings(4)
    try:
        with kzg.PolySettings(fs) as ps:
            chunk = ps.info()[1]
            ln = 64 * 64 * chunk + 3 * chunk + 5
            p = _once(("evalp", ln), lambda: [rnd.randrange(R) for _ in range(ln)])
            xs = [R - 1, 3, 0x1234567890ABCDEF]
            assert _ints(ps.eval(_fr(p), ln, 1, _fr(xs), 3), 3) == [P.evaluate(p, x) for x in xs]
    finally:
        fs.close()


# ---------------------------------------------------------------- scale
def test_scale_and_unscale(kzg):
    rnd = random.Random(13)
    fs = kzg.FFTSettings(4)
    try:
        with kzg.PolySettings(fs) as ps:
            for ln in (1, 2, 300):
                polys = [[rnd.randrange(R) for _ in range(ln)] for _ in range(2)]
                scaled = ps.scale(_flat(polys), ln, 2)
                assert _ints(scaled, 2 * ln) == [v for p in polys for v in P.scale(p)], ln
                assert _ints(ps.scale(scaled, ln, 2, inverse=True), 2 * ln) == [v for p in polys for v in p], ln
                up = _ints(ps.scale(_flat(polys), ln, 2, inverse=True), 2 * ln)
                assert up == [v for p in polys for v in P.unscale(p)], ln
                assert _ints(scaled, 1)[0] == polys[0][0] * pow(5, R - 2, R) % R and up[0] == polys[0][0] * 5 % R
    finally:
        fs.close()


# ---------------------------------------------------------------- mul
@pytest.mark.parametrize("la", [1, 63, 64, 65, 200])
def test_mul_forms_agree_with_the_model_around_the_thresholds(kzg, la):
    rnd = random.Random(100 + la)
    fs = kzg.FFTSettings(10)
    try:
        with kzg.PolySettings(fs) as ps:
            mul_max = ps.info()[2]
            for lb in sorted({1, 63, 64, 65, 200, mul_max, mul_max + 1}):
                a, b = _rand(rnd, la), _rand(rnd, lb)
                full = _once(("mul", la, lb), lambda: P.mul_direct(a, b, la + lb - 1))
                tlen = P.next_pow_of_2(la + lb - 1)
                for out_len in sorted({1, max(1, (la + lb - 1) // 2), la + lb - 1, la + lb + 6, 2 * tlen + 3}):
                    want = _fit(full, out_len)
                    for form in (0, 1, 2):
                        got = _ints(ps.mul(_fr(a), la, _fr(b), lb, out_len, 1, form), out_len)
                        assert got == want, (la, lb, out_len, form)
    finally:
        fs.close()


def test_mul_with_an_8192_point_transform(kzg):
    rnd = random.Random(14)
    fs = kzg.FFTSettings(13)
    try:
        with kzg.PolySettings(fs) as ps:
            la, lb = 3000, 1200
            assert ps.transform_len("mul", la, lb, la + lb - 1) == 8192
            a, b = _rand(rnd, la), _rand(rnd, lb)
            want = _once(("mul8192",), lambda: P.mul_fft(a, b, la + lb - 1))
            for form in (0, 2):
                got = _ints(ps.mul(_fr(a), la, _fr(b), lb, la + lb - 1, 1, form), la + lb - 1)
                assert got == want, form
                for _ in range(3):
                    z = rnd.randrange(R)
                    assert P.evaluate(a, z) * P.evaluate(b, z) % R == P.evaluate(got, z)
            # cut below the operands: the transform shrinks with the output
            assert ps.transform_len("mul", la, lb, 1000) == 2048
            assert _ints(ps.mul(_fr(a), la, _fr(b), lb, 1000, 1, 2), 1000) == want[:1000]
    finally:
        fs.close()


def test_mul_empty_operands_and_batches(kzg):
    rnd = random.Random(15)
    fs = kzg.FFTSettings(10)
    try:
        with kzg.PolySettings(fs) as ps:
            a = _rand(rnd, 7)
            assert _ints(ps.mul(_fr(a), 7, _fr([]), 0, 5, 1), 5) == [0] * 5
            assert _ints(ps.mul(_fr([]), 0, _fr(a), 7, 5, 2), 10) == [0] * 10
            for la, lb, out_len in ((70, 90, 159), (70, 90, 100), (5, 9, 20)):
                A = [_rand(rnd, la) for _ in range(4)]
                B = [_rand(rnd, lb) for _ in range(4)]
                for form in (0, 1, 2):
                    batch = bytes(ps.mul(_flat(A), la, _flat(B), lb, out_len, 4, form))
                    single = b"".join(bytes(ps.mul(_fr(x), la, _fr(y), lb, out_len, 1, form)) for x, y in zip(A, B))
                    assert batch == single, (la, lb, out_len, form)
                assert _ints(batch, out_len) == _fit(P.mul_direct(A[0], B[0], la + lb - 1), out_len)
    finally:
        fs.close()


# ---------------------------------------------------------------- inverse
def test_inverse_reference_series_and_constants(kzg):
    fs = kzg.FFTSettings(6)
    try:
        with kzg.PolySettings(fs) as ps:
            assert _ints(ps.inverse(_fr([1, R - 1]), 2, 16), 16) == [1] * 16
            assert _ints(ps.inverse(_fr([1, 1]), 2, 16), 16) == [1 if i % 2 == 0 else R - 1 for i in range(16)]
            assert _ints(ps.inverse(_fr([7]), 1, 5), 5) == [pow(7, R - 2, R), 0, 0, 0, 0]
            assert _ints(ps.inverse(_fr([7, 9]), 2, 1), 1) == [pow(7, R - 2, R)]
    finally:
        fs.close()


def test_inverse_against_the_recurrence_around_the_direct_switch(kzg):
    rnd = random.Random(16)
    fs = kzg.FFTSettings(11)
    try:
        with kzg.PolySettings(fs) as ps:
            inv_max = ps.info()[3]
            b = [rnd.randrange(1, R)] + _rand(rnd, 39)
            want = _once(("inv40",), lambda: P.inverse_recurrence(b, 1000))
            for L in sorted({1, 2, 3, 5, 17, inv_max, inv_max + 1, 129, 1000}):
                assert _ints(ps.inverse(_fr(b), 40, L), L) == want[:L], L
            # lb > out_len: only the first out_len coefficients of b matter
            other = b[:17] + [rnd.randrange(R) for _ in range(23)]
            assert bytes(ps.inverse(_fr(other), 40, 17)) == bytes(ps.inverse(_fr(b), 40, 17))
            assert _ints(ps.inverse(_fr(other), 40, 17), 17) == want[:17]
            wide = [rnd.randrange(1, R)] + _rand(rnd, 299)
            changed = wide[:100] + [rnd.randrange(R) for _ in range(200)]
            assert bytes(ps.inverse(_fr(wide), 300, 100)) == bytes(ps.inverse(_fr(changed), 300, 100))
            assert _ints(ps.inverse(_fr(wide), 300, 100), 100) == P.inverse_recurrence(wide, 100)
    finally:
        fs.close()


@pytest.mark.parametrize("lb,L", [(40, 5000), (1200, 1200)])
def test_inverse_times_b_is_one(kzg, lb, L):
    rnd = random.Random(17 + lb)
    fs = kzg.FFTSettings(14)
    try:
        with kzg.PolySettings(fs) as ps:
            b = [rnd.randrange(1, R)] + _rand(rnd, lb - 1)
            c = _ints(ps.inverse(_fr(b), lb, L), L)
            assert P.mul_fft(b, c, L) == [1] + [0] * (L - 1)
    finally:
        fs.close()


def test_inverse_flags_a_zero_constant_term_in_the_batch(kzg):
    rnd = random.Random(18)
    fs = kzg.FFTSettings(9)
    try:
        with kzg.PolySettings(fs) as ps:
            polys = [[rnd.randrange(1, R)] + _rand(rnd, 9) for _ in range(5)]
            for L in (1, 20, 100):
                got = _ints(ps.inverse(_flat(polys), 10, L, 5), 5 * L)
                assert got == [v for p in polys for v in P.inverse_recurrence(p, L)]
            polys[2][0] = 0
            for L in (1, 20, 100):
                with pytest.raises(kzg.KzgAmdError, match="First coefficient") as e:
                    ps.inverse(_flat(polys), 10, L, 5)
                assert e.value.code == 3
            for args, code in (((_fr([1]), 1, 0), 1), ((_fr([]), 0, 4), 2)):
                with pytest.raises(kzg.KzgAmdError) as e:
                    ps.inverse(*args)
                assert e.value.code == code
    finally:
        fs.close()


# ---------------------------------------------------------------- div
DIV_TABLE = [
    ([-1, 0, 1], [1, 1], [-1, 1]),
    ([18, 9, -11, 12], [3, 4], [6, -5, 3]),
    ([1, 1], [-1, 0, 2], []),
    ([30, 20, 10], [10], [3, 2, 1]),
    ([0, 1, 1], [1, 1], [0, 1]),
    ([1, 1, 1], [1], [1, 1, 1]),
    ([1, 1, 1], [1, 0], [1, 1, 1]),
]


def test_div_reference_table_and_error_codes(kzg):
    L = kzg.lib()
    fs = kzg.FFTSettings(6)
    try:
        with kzg.PolySettings(fs) as ps:
            for row in range(6):
                a, b, q = ([c % R for c in v] for v in DIV_TABLE[row])
                got = ps.div(_fr(a), len(a), _fr(b), len(b))
                assert len(bytes(got)) == 32 * len(q) and _ints(got, len(q)) == q, row
            a, b, _ = DIV_TABLE[6]
            with pytest.raises(kzg.KzgAmdError, match="Highest coefficient must be non-zero") as e:
                ps.div(_fr(a), 3, _fr(b), 2)
            assert e.value.code == 2
            with pytest.raises(kzg.KzgAmdError, match="Can't divide by zero") as e:
                ps.div(_fr([1, 1]), 2, _fr([]), 0)
            assert e.value.code == 1
            # a zero highest coefficient of one divisor of a batch, constant divisors included
            assert L.kzgamd_poly_div(ps.handle, _fr([0] * 6), _fr([1, 2, 3, 4, 5, 6]), 3, _fr([1, 0]), 1, 2) == 2
            # la < lb: ok, nothing written
            q = _fr([77] * 4)
            sentinel = bytes(q)
            assert L.kzgamd_poly_div(ps.handle, q, _fr([1, 1]), 2, _fr([R - 1, 0, 2]), 3, 1) == 0
            assert bytes(q) == sentinel
    finally:
        fs.close()


@pytest.mark.parametrize("lb", [1, 2, 3, 127, 128, 129])
def test_div_by_construction_around_the_reference_thresholds(kzg, lb):
    fs = kzg.FFTSettings(11)
    try:
        with kzg.PolySettings(fs) as ps:
            a, b, q = _by_construction(lb, 700, lb)
            assert _ints(ps.div(_fr(a), 700, _fr(b), lb), 700 - lb + 1) == q
            if lb in (3, 129):
                assert q == _once(("long_div", lb), lambda: P.long_div(a, b))   # the construction itself, once
    finally:
        fs.close()


def test_div_whose_transforms_cross_the_tile(kzg):
    fs = kzg.FFTSettings(14)
    try:
        with kzg.PolySettings(fs) as ps:
            assert ps.transform_len("div", 9000, 4097, 0) > 4096
            a, b, q = _by_construction(21, 9000, 4097)
            assert _ints(ps.div(_fr(a), 9000, _fr(b), 4097), len(q)) == q
    finally:
        fs.close()


def test_div_at_the_reference_bench_shape(kzg):
    la, lb = 1 << 15, 1 << 14
    fs = kzg.FFTSettings(16)
    try:
        with kzg.PolySettings(fs) as ps:
            a, b, q = _by_construction(22, la, lb)
            assert _ints(ps.div(_fr(a), la, _fr(b), lb), len(q)) == q
    finally:
        fs.close()


def test_div_batch_equals_single_calls(kzg):
    fs = kzg.FFTSettings(11)
    try:
        with kzg.PolySettings(fs) as ps:
            for la, lb in ((700, 129), (300, 1), (90, 40)):
                cases = [_by_construction(30 + i, la, lb) for i in range(3)]
                batch = bytes(ps.div(_flat([c[0] for c in cases]), la, _flat([c[1] for c in cases]), lb, 3))
                single = b"".join(bytes(ps.div(_fr(a), la, _fr(b), lb)) for a, b, _ in cases)
                assert batch == single, (la, lb)
                assert _ints(batch, 3 * (la - lb + 1)) == [v for c in cases for v in c[2]], (la, lb)
    finally:
        fs.close()


# ---------------------------------------------------------------- width
def test_a_handle_exactly_as_wide_as_transform_len_succeeds_and_half_of_it_returns_4(kzg):
    L = kzg.lib()
    rnd = random.Random(19)
    a200, b200 = _rand(rnd, 200), _rand(rnd, 200)
    b40 = [rnd.randrange(1, R)] + _rand(rnd, 39)
    da, db, dq = _by_construction(40, 700, 129)
    T = kzg.PolySettings.transform_len
    calls = [
        (T("mul", 200, 200, 399), 399, lambda h, out: L.kzgamd_poly_mul(h, out, _fr(a200), 200, _fr(b200), 200, 399, 1, 2),
         lambda: P.mul_direct(a200, b200, 399)),
        (T("inverse", 0, 40, 1000), 1000, lambda h, out: L.kzgamd_poly_inverse(h, out, _fr(b40), 40, 1000, 1),
         lambda: P.inverse_recurrence(b40, 1000)),
        (T("div", 700, 129, 0), 572, lambda h, out: L.kzgamd_poly_div(h, out, _fr(da), 700, _fr(db), 129, 1), lambda: dq),
    ]
    for i, (width, count, call, want) in enumerate(calls):
        assert width >= 512 and width & (width - 1) == 0
        for w, code in ((width, 0), (width // 2, 4)):
            fs = kzg.FFTSettings(w.bit_length() - 1)
            try:
                with kzg.PolySettings(fs) as ps:
                    assert ps.info()[0] == w
                    out = _fr([77] * count)
                    sentinel = bytes(out)
                    assert call(ps.handle, out) == code, (i, w)
                    if code == 0:
                        assert _ints(out, count) == _once(("width", i), want), i
                    else:
                        assert bytes(out) == sentinel, i
            finally:
                fs.close()


# ---------------------------------------------------------------- empty calls
def test_empty_calls_write_nothing_and_null_arguments_are_refused(kzg):
    L = kzg.lib()
    fs = kzg.FFTSettings(6)
    try:
        with kzg.PolySettings(fs) as ps:
            h = ps.handle
            buf, p = _fr([77] * 8), _fr([1, 2, 3, 4])
            sentinel = bytes(buf)
            assert L.kzgamd_poly_eval(h, buf, p, 4, 0, p, 1) == 0
            assert L.kzgamd_poly_eval(h, buf, p, 4, 1, None, 0) == 0
            assert L.kzgamd_poly_eval(h, None, None, 4, 0, None, 0) == 0
            assert L.kzgamd_poly_scale(h, buf, p, 4, 0, 0) == 0 and L.kzgamd_poly_scale(h, buf, p, 0, 1, 0) == 0
            assert L.kzgamd_poly_mul(h, buf, p, 2, p, 2, 3, 0, 0) == 0 and L.kzgamd_poly_mul(h, buf, p, 2, p, 2, 0, 1, 0) == 0
            assert L.kzgamd_poly_inverse(h, buf, p, 4, 4, 0) == 0
            assert L.kzgamd_poly_div(h, buf, p, 4, p, 2, 0) == 0
            assert bytes(buf) == sentinel
            assert L.kzgamd_poly_eval(h, None, p, 4, 1, p, 1) == -1
            assert L.kzgamd_poly_eval(h, buf, None, 4, 1, p, 1) == -1
            assert L.kzgamd_poly_eval(h, buf, p, 4, 1, None, 1) == -1
            assert L.kzgamd_poly_scale(h, None, p, 4, 1, 0) == -1 and L.kzgamd_poly_scale(h, buf, None, 4, 1, 0) == -1
            assert L.kzgamd_poly_mul(h, None, p, 2, p, 2, 3, 1, 0) == -1
            assert L.kzgamd_poly_mul(h, buf, None, 2, p, 2, 3, 1, 0) == -1
            assert L.kzgamd_poly_mul(h, buf, p, 2, None, 2, 3, 1, 0) == -1
            assert L.kzgamd_poly_mul(h, buf, p, 2, p, 2, 3, 1, 3) == -1          # no such form
            assert L.kzgamd_poly_inverse(h, None, p, 4, 4, 1) == -1 and L.kzgamd_poly_inverse(h, buf, None, 4, 4, 1) == -1
            assert L.kzgamd_poly_div(h, None, p, 4, p, 2, 1) == -1
            assert L.kzgamd_poly_div(h, buf, None, 4, p, 2, 1) == -1 and L.kzgamd_poly_div(h, buf, p, 4, None, 2, 1) == -1
            assert bytes(buf) == sentinel
            # eval of empty polynomials: zeros
            assert _ints(ps.eval(_fr([]), 0, 2, _fr([3, 4]), 2), 4) == [0] * 4
        err = C.c_int(77)
        assert not L.kzgamd_poly_new(None, None, C.byref(err)) and err.value == -1
        cfg = kzg.make_config(tuning="nonsense=1")
        assert not L.kzgamd_poly_new(fs.handle, C.byref(cfg), C.byref(err)) and err.value == -2
    finally:
        fs.close()


# ---------------------------------------------------------------- lifecycle and threads
def test_lifecycle_returns_hbm_and_threads_share_a_handle(kzg):
    import torch

    rnd = random.Random(20)
    fs = kzg.FFTSettings(11)
    try:
        A = [_rand(rnd, 300) for _ in range(3)]
        B = [[rnd.randrange(1, R)] + _rand(rnd, 99) for _ in range(3)]
        fa, fb = _flat(A), _flat(B)

        def use(ps):
            return (bytes(ps.mul(fa, 300, fb, 100, 399, 3)), bytes(ps.inverse(fb, 100, 300, 3)), bytes(ps.div(fa, 300, fb, 100, 3)),
                    bytes(ps.eval(fa, 300, 3, fb, 2)))

        def cycle():
            with kzg.PolySettings(fs) as ps:
                return use(ps)

        want = cycle()
        assert _ints(want[0], 399) == P.mul_direct(A[0], B[0], 399)
        assert _ints(want[1], 300) == P.inverse_recurrence(B[0], 300)
        assert _ints(want[2], 201) == P.long_div(A[0], B[0])
        assert _ints(want[3], 2) == [P.evaluate(A[0], B[0][0]), P.evaluate(A[0], B[0][1])]
        torch.cuda.synchronize()
        base, _ = torch.cuda.mem_get_info(0)
        deltas = []
        for _ in range(10):
            assert cycle() == want
            torch.cuda.synchronize()
            free, _ = torch.cuda.mem_get_info(0)
            deltas.append((base - free) / MB)
            assert base - free <= 8 * MB, deltas
        print("poly lifecycle: HBM delta MB per cycle:", ["%.2f" % d for d in deltas])

        with kzg.PolySettings(fs) as ps:
            failures = []

            def work(t):
                try:
                    for _ in range(4):
                        assert use(ps) == want
                except Exception as e:  # noqa: BLE001
                    failures.append((t, repr(e)))

            ts = [threading.Thread(target=work, args=(t,)) for t in range(4)]
            for th in ts:
                th.start()
            for th in ts:
                th.join()
            assert failures == []
    finally:
        fs.close()
