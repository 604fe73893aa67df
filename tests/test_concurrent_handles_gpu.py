"""Concurrent callers on ONE B1 / B2 handle (calls of the same kind and length are combined into batched launches below
the seam: combine.h combined_call, which msm.hip msm_run_host_combined and ntt.hip run_host_combined queue their requests
on).  The reference shares its handles between rayon workers: SpparkPrecomputation
is Send + Sync and lives in an Arc (kzg/src/msm/sppark.rs:24-44), verify_blob_kzg_proof_batch calls the MSM from
par_chunks (kzg/src/eip_4844.rs:781-805), FFT settings are shared by reference.  Sixteen threads per handle, every
result against the oracle: mult_pippenger_prepared (whose concurrent calls are combined into one launch),
ntt_fr / das_fft_extension, fft_g1.  Sixty-four threads per handle, more than it has staging slots (48 / 40): the
callers that find the pool empty."""
import ctypes as C
import random
import threading

import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu
THREADS = 16


def compressed(L, p):
    buf = C.create_string_buffer(48)
    g = O.G1()
    C.memmove(C.byref(g), C.byref(p), 144)
    L.og1_compress(buf, C.byref(g))
    return buf.raw


def fr_bulk(vals):
    arr = (O.Fr * len(vals))()
    raw = b"".join(((v << 256) % O.R).to_bytes(32, "little") for v in vals)
    C.memmove(arr, raw, len(raw))
    return arr


def run_threads(work, threads=THREADS):
    """work(t) on `threads` threads released together; returns the list of failures the threads recorded"""
    failures = []
    gate = threading.Barrier(threads)

    def body(t):
        try:
            gate.wait()
            work(t)
        except Exception as e:  # noqa: BLE001
            failures.append((t, repr(e)))

    ts = [threading.Thread(target=body, args=(t,)) for t in range(threads)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    return failures


def test_sixteen_threads_share_one_prepared_msm_handle(kzg, oracle, oracle_settings):
    L = oracle.lib()
    n = 4096
    pts = oracle_settings.g1_lagrange_brp
    h = kzg.prepare_multi_scalar_mult(pts, n)
    lengths = [4096, 4096, 4096, 1000, 4096, 8, 4096, 77]  # equal lengths are combined, the others run between them
    calls = len(lengths)
    inputs = {}
    for t in range(THREADS):
        rnd = random.Random(9000 + t)
        for k in range(calls):
            m = lengths[(k + t) % calls]
            vals = [rnd.randrange(O.R) for _ in range(m)]
            if k == 3:
                vals[0] = 0
                vals[-1] = O.R - 1
            inputs[(t, k)] = (m, fr_bulk(vals))
    got = {}

    def work(t):
        for k in range(calls):
            m, sc = inputs[(t, k)]
            got[(t, k)] = compressed(L, kzg.multi_scalar_mult_prepared(h, sc, m))

    assert run_threads(work) == []
    for (t, k), (m, sc) in inputs.items():
        exp = O.G1()
        L.omsm_affine(C.byref(exp), pts, sc, m)
        assert got[(t, k)] == compressed(L, exp), (t, k, m)
    # a failing call among good ones fails alone: more scalars than the handle holds
    bad = fr_bulk([1] * (n + 1))

    def work2(t):
        if t == 5:
            with pytest.raises(kzg.KzgAmdError):
                kzg.multi_scalar_mult_prepared(h, bad, n + 1)
        else:
            m, sc = inputs[(t, 0)]
            assert compressed(L, kzg.multi_scalar_mult_prepared(h, sc, m)) == got[(t, 0)]

    assert run_threads(work2) == []
    h.close()


def test_sixteen_threads_share_one_ntt_handle(kzg, oracle):
    L = oracle.lib()
    scale = 13
    fs = kzg.FFTSettings(scale)
    ofs = O.FFTSettings()
    assert L.offt_settings_new(C.byref(ofs), scale) == 0
    sizes = [4096, 8192, 64, 4096, 1, 1024]
    inputs = {}
    for t in range(THREADS):
        rnd = random.Random(7000 + t)
        for k, n in enumerate(sizes):
            inputs[(t, k)] = (n, (t + k) % 2 == 1, fr_bulk([rnd.randrange(O.R) for _ in range(n)]))
    got = {}

    def work(t):
        for k in range(len(sizes)):
            n, inv, data = inputs[(t, k)]
            got[(t, k)] = bytes(fs.fft_fr(data, n, inverse=inv))[: 32 * n]
            if 2 <= n <= 4096:
                got[(t, k, "das")] = bytes(fs.das_fft_extension(data, n))[: 32 * n]

    assert run_threads(work) == []
    for (t, k), (n, inv, data) in inputs.items():
        exp = (O.Fr * n)()
        assert L.offt_fr(C.byref(ofs), exp, data, n, 1 if inv else 0) == 0
        assert got[(t, k)] == bytes(exp), (t, k, n, inv)
        if 2 <= n <= 4096:
            odds = (O.Fr * n)()
            assert L.odas_fft_extension(C.byref(ofs), odds, data, n) == 0
            assert got[(t, k, "das")] == bytes(odds), (t, k, n)
    # the same calls with the combining off (tuning key combine=0: every call on the handle's mutex): the same bytes
    fs2 = kzg.FFTSettings(scale, kzg.make_config(tuning={"combine": 0}))
    got2 = {}

    def work_plain(t):
        for k in range(len(sizes)):
            n, inv, data = inputs[(t, k)]
            got2[(t, k)] = bytes(fs2.fft_fr(data, n, inverse=inv))[: 32 * n]

    assert run_threads(work_plain) == []
    assert all(got2[key] == got[key] for key in got2)
    fs2.close()
    # errors keep their codes through the combined path, and a call longer than the combining limit takes the plain one
    with pytest.raises(kzg.KzgAmdError, match="power-of-two"):
        fs.fft_fr(inputs[(0, 0)][2], 12)
    big = kzg.FFTSettings(15)
    n = 1 << 15
    rnd = random.Random(5)
    data = fr_bulk([rnd.randrange(O.R) for _ in range(n)])
    ofs15 = O.FFTSettings()
    assert L.offt_settings_new(C.byref(ofs15), 15) == 0
    exp = (O.Fr * n)()
    assert L.offt_fr(C.byref(ofs15), exp, data, n, 0) == 0
    assert bytes(big.fft_fr(data, n))[: 32 * n] == bytes(exp)
    big.close()
    L.offt_settings_free(C.byref(ofs15))
    fs.close()
    L.offt_settings_free(C.byref(ofs))


def test_sixteen_threads_share_one_fft_g1_handle(kzg, oracle):
    L = oracle.lib()
    scale = 8
    fs = kzg.FFTSettings(scale)
    ofs = O.FFTSettings()
    assert L.offt_settings_new(C.byref(ofs), scale) == 0
    g = O.G1()
    L.og1_generator(C.byref(g))
    rnd = random.Random(81)
    pool = []
    for _ in range(40):
        p = O.G1()
        k = O.fr_from_int(rnd.randrange(1, O.R))
        L.og1_mul(C.byref(p), C.byref(g), C.byref(k))
        pool.append(p)
    sizes = [64, 16, 256, 64]
    inputs = {}
    for t in range(THREADS):
        for k, n in enumerate(sizes):
            data = (O.G1 * n)()
            for i in range(n):
                data[i] = O.G1() if (i + t) % 11 == 0 else pool[rnd.randrange(len(pool))]
            inputs[(t, k)] = (n, (t + k) % 2 == 0, data)
    got = {}

    def work(t):
        for k in range(len(sizes)):
            n, inv, data = inputs[(t, k)]
            out = fs.fft_g1(data, n, inverse=inv)
            got[(t, k)] = [compressed(L, out[i]) for i in range(n)]

    assert run_threads(work) == []
    for (t, k), (n, inv, data) in inputs.items():
        exp = (O.G1 * n)()
        assert L.offt_g1(C.byref(ofs), exp, data, n, 1 if inv else 0) == 0
        assert got[(t, k)] == [compressed(L, exp[i]) for i in range(n)], (t, k, n, inv)
    fs.close()
    L.offt_settings_free(C.byref(ofs))


def test_calls_at_and_beyond_the_combining_limit_share_one_handle(kzg, oracle):
    """Calls of up to 2^16 scalars are combined (a page-locked slot holds exactly that many), longer ones take the
    handle's own stream under its mutex (msm.hip: COMBINE_NMAX): both kinds at once on one handle, each against the
    oracle's Pippenger on the same points."""
    import torch

    L = oracle.lib()
    lim = 1 << 16
    n = lim + 64
    d_pts = torch.empty(n * 96, dtype=torch.uint8, device="cuda")
    kzg.generate_points(d_pts.data_ptr(), n, 21, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pts = (O.G1Affine * n).from_buffer_copy(d_pts.cpu().numpy().tobytes())
    h = kzg.prepare_multi_scalar_mult(pts, n, kzg.make_config(table_budget_gb=8))
    rnd = random.Random(33)
    want, scalars = {}, {}
    for m in (lim, n, lim - 1):
        vals = [rnd.randrange(O.R) for _ in range(m)]
        vals[0], vals[-1] = 0, O.R - 1
        exp = O.G1()
        L.omsm_tiling_pippenger(C.byref(exp), pts, b"".join(v.to_bytes(32, "little") for v in vals), m)
        want[m] = compressed(L, exp)
        scalars[m] = fr_bulk(vals)  # Montgomery form, what mult_pippenger_prepared takes
    order = [lim, n, lim - 1, n]
    got = {}

    def work(t):
        for k in range(3):
            m = order[(t + k) % len(order)]
            got[(t, k)] = (m, compressed(L, kzg.multi_scalar_mult_prepared(h, scalars[m], m)))

    assert run_threads(work) == []
    assert len(got) == 3 * THREADS
    for key, (m, c) in got.items():
        assert c == want[m], (key, m)
    h.close()


MANY = 64  # callers per handle in the two tests below: more than its staging slots


def test_more_callers_than_slots_share_one_prepared_msm_handle(kzg, oracle, oracle_settings):
    """64 threads, 8 calls each, on one prepared handle of 64 points whose pool holds 48 page-locked slots: a caller that
    finds the pool empty queues its own (pageable) scalars, and a batch with such a request copies per request instead
    of gathering from the slots (msm.hip: msm_run_combined_batch).  Whether a given run empties the pool is up to the
    scheduler; that an empty pool gives no slot is checked deterministically on the CPU (test_combine_queue_cpu.py).
    Every result against what a combine=0 handle over the same points returns for the same scalars, one call after
    the other, and one call of each length against the oracle."""
    L = oracle.lib()
    n = 64
    pts = oracle_settings.g1_lagrange_brp
    h = kzg.prepare_multi_scalar_mult(pts, n, kzg.make_config(table_budget_gb=0.5))
    plain = kzg.prepare_multi_scalar_mult(pts, n, kzg.make_config(table_budget_gb=0.5, tuning={"combine": 0}))
    calls = 8
    inputs, want = {}, {}
    for t in range(MANY):
        rnd = random.Random(4100 + t)
        for k in range(calls):
            m = 64 if (t + k) % 2 == 0 else 17
            inputs[(t, k)] = (m, fr_bulk([rnd.randrange(O.R) for _ in range(m)]))
    for key, (m, sc) in inputs.items():
        want[key] = compressed(L, kzg.multi_scalar_mult_prepared(plain, sc, m))
    for key in ((0, 0), (0, 1)):
        m, sc = inputs[key]
        exp = O.G1()
        L.omsm_affine(C.byref(exp), pts, sc, m)
        assert want[key] == compressed(L, exp), (key, m)
    got = {}

    def work(t):
        for k in range(calls):
            m, sc = inputs[(t, k)]
            got[(t, k)] = compressed(L, kzg.multi_scalar_mult_prepared(h, sc, m))

    assert run_threads(work, MANY) == []
    assert len(got) == MANY * calls
    for key in inputs:
        assert got[key] == want[key], key
    plain.close()
    h.close()


def test_more_callers_than_slots_share_one_ntt_handle(kzg):
    """64 threads, 8 calls each, on one scale-5 handle whose pool holds 40 page-locked slots: a caller that finds the pool
    empty takes the plain path on the handle's mutex, beside the batches of the others (ntt.hip: run_host_combined).
    Whether a given run empties the pool is up to the scheduler; that an empty pool gives no slot is checked
    deterministically on the CPU (test_combine_queue_cpu.py).  Lengths 32 and 8, kinds rotating over forward, inverse
    and DAS extension — whose list is half the domain at most, so it takes 16 where the others take 32.  Every result
    against the bytes of a combine=0 handle, one call after the other."""
    scale = 5
    fs = kzg.FFTSettings(scale)
    plain = kzg.FFTSettings(scale, kzg.make_config(tuning={"combine": 0}))
    calls = 8

    def call(h, kind, n, data):
        out = h.das_fft_extension(data, n) if kind == 2 else h.fft_fr(data, n, inverse=kind == 1)
        return bytes(out)[: 32 * n]

    inputs, want = {}, {}
    for t in range(MANY):
        rnd = random.Random(5200 + t)
        for k in range(calls):
            kind = (t + k) % 3
            n = 32 if k % 2 == 0 else 8
            if kind == 2 and n == 32:
                n = 16
            inputs[(t, k)] = (kind, n, fr_bulk([rnd.randrange(O.R) for _ in range(n)]))
    for key, (kind, n, data) in inputs.items():
        want[key] = call(plain, kind, n, data)
    assert len({(kind, n) for kind, n, _ in inputs.values()}) == 6
    got = {}

    def work(t):
        for k in range(calls):
            kind, n, data = inputs[(t, k)]
            got[(t, k)] = call(fs, kind, n, data)

    assert run_threads(work, MANY) == []
    assert len(got) == MANY * calls
    for key in inputs:
        assert got[key] == want[key], key
    plain.close()
    fs.close()
