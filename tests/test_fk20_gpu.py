"""Generic FK20 data-availability proofs on the GPU (kzgamd_fk20_new / kzgamd_fk20_da): FK20SingleSettings and
FK20MultiSettings of the reference for any polynomial length and chunk length, several polynomials per call.

Three anchors, none of them the code under test:
  A. the closed form with the known secret (tests/fk20_model.py, pinned on the CPU by tests/test_fk20_model_cpu.py):
     the setup is [s^i]G for the reference's public SECRET, so proof j of the optimized output must be
     [(p(s) - I_j(s)) / (s^l - w^j)]G — every position is checked, [scalar]G by the CPU oracle;
  B. the reference's compute_cells_and_kzg_proofs vectors: a handle over the mainnet monomial setup with n2 = 8192,
     chunk_len = 64 must give the 128 proofs of every valid vector byte for byte;
  C. form against form (a scalar multiplication per product / the wide fixed-base table) and batch against single.

Table legs get an explicit table budget and are skipped, with the reason, only where the free HBM cannot hold the
table; the direct form is never skipped."""
import ctypes as C
import hashlib
import random
import threading

import pytest

import fk20_model as M
import oracle_ffi as O

pytestmark = pytest.mark.gpu
R = M.R
GB = 1e9

_setup_cache = {}
_expected_cache = {}


def _setup(npoints):
    """[s^i]G, i < npoints, as blst_p1 (the oracle's Jacobian layout is blst's); grown once per session"""
    L = O.lib()
    have = _setup_cache.get("pts", [])
    if len(have) < npoints:
        g = O.G1()
        L.og1_generator(C.byref(g))
        sp = pow(M.SECRET, len(have), R)
        for _ in range(len(have), npoints):
            out = O.G1()
            L.og1_mul(C.byref(out), C.byref(g), C.byref(O.fr_from_int(sp)))
            have.append(bytes(out))
            sp = sp * M.SECRET % R
        _setup_cache["pts"] = have
    return b"".join(have[:npoints])


def _expected(key, scalars):
    """[scalar]G for every scalar (None for zero: the identity), cached per case"""
    if key not in _expected_cache:
        L = O.lib()
        g = O.G1()
        L.og1_generator(C.byref(g))
        out = []
        for v in scalars:
            if v == 0:
                out.append(None)
                continue
            e = O.G1()
            L.og1_mul(C.byref(e), C.byref(g), C.byref(O.fr_from_int(v)))
            out.append(e)
        _expected_cache[key] = out
    return _expected_cache[key]


def _fr_bulk(vals):
    raw = b"".join(((v << 256) % R).to_bytes(32, "little") for v in vals)
    arr = (O.Fr * (len(vals) or 1))()
    C.memmove(arr, raw, len(raw))
    return arr


def _root(fs, order):
    """the handle's root of that order: roots_of_unity[max_width / order], out of Montgomery form"""
    r, _, _ = fs.roots()
    v = int.from_bytes(bytes(r[fs.max_width // order]), "little")
    return v * pow(1 << 256, R - 2, R) % R


def _points(out, count):
    raw = bytes(out)
    pts = []
    for i in range(count):
        g = O.G1()
        C.memmove(C.byref(g), raw[144 * i: 144 * (i + 1)], 144)
        pts.append(g)
    return pts


def _assert_points(got, exp, what):
    L = O.lib()
    assert len(got) == len(exp)
    for j, (g, e) in enumerate(zip(got, exp)):
        if e is None:
            assert L.og1_is_inf(C.byref(g)), (what, j, "expected the identity")
        else:
            assert not L.og1_is_inf(C.byref(g)) and L.og1_equal(C.byref(g), C.byref(e)), (what, j)


def _free_gb():
    import torch

    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0] / GB


def _table_min_gb(n2):
    """the smallest wide table over the 2n = n2 points of a handle: 13 rows of 2^9 slots of 128 B per point"""
    return n2 * 512 * 13 * 128 / GB


def _config(kzg, form, n2):
    """direct: fk20_table=0.  table: fk20_table=1 with a budget just above the smallest table, or a skip with the reason
    when the free HBM (less the 12 GB the engine keeps clear, and the call's own workspace) cannot hold it."""
    if form == "direct":
        return kzg.make_config(tuning={"fk20_table": 0})
    need = max(_table_min_gb(n2) * 1.02, 0.001)
    free = _free_gb()
    if (free - 12) / 1.05 < need + 1:
        pytest.skip("table form of n2 = %d needs %.1f GB of HBM for its table, %.1f GB are free" % (n2, need, free))
    return kzg.make_config(table_budget_gb=need, tuning={"fk20_table": 1})


def _make(kzg, fs, n2, l, form, setup=None, num=None):
    n = n2 // 2
    if setup is None:
        num = max(n - l, 1)
        setup = _setup(num)
    fk = kzg.FK20Settings(fs, setup, num, n2, l, _config(kzg, form, n2))
    assert fk.info() == (n2, l, 1 if form == "direct" else 2)
    return fk


def _closed(fs, p, l):
    return M.fk20_closed_form(p, l, M.SECRET, _root(fs, 2 * len(p) // l))


def _check_case(kzg, scale, p, l, form, name, orders=(True, False)):
    n = len(p)
    k2 = 2 * n // l
    fs = kzg.FFTSettings(scale)
    try:
        exp = _expected((name, scale, l), _closed(fs, p, l))
        with _make(kzg, fs, 2 * n, l, form) as fk:
            opt = _points(fk.data_availability(_fr_bulk(p), 1, optimized=True), k2)
            _assert_points(opt, exp, name + " optimized")
            if False in orders:
                brp = _points(fk.data_availability(_fr_bulk(p), 1, optimized=False), k2)
                bits = k2.bit_length() - 1
                assert [bytes(brp[M.brev(i, bits)]) for i in range(k2)] == [bytes(x) for x in opt], name
    finally:
        fs.close()


FORMS = ["direct", "table"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("scale", [5, 8])
def test_fk_single_and_strided(kzg, form, scale):
    """fk_single (scale 5) and fk_single_strided (the same polynomial over an NTT handle of scale 8)"""
    _check_case(kzg, scale, M.fk_single_poly(), 1, form, "fk_single")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("l,n", [(1, 512), (16, 512), (16, 16), (32, 64)])
def test_fk_multi_reference_cases(kzg, form, l, n):
    """fk_multi_chunk_len_1_512, _16_512, _16_16 with the reference's polynomial, and (32, 64)"""
    _check_case(kzg, (2 * n).bit_length() - 1, M.fk_multi_poly(n, l), l, form, "fk_multi_%d_%d" % (l, n))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("l,n", [(1, 256), (16, 512)])
def test_random_full_width_coefficients(kzg, form, l, n):
    rnd = random.Random(1000 * l + n)
    _check_case(kzg, (2 * n).bit_length() - 1, [rnd.randrange(R) for _ in range(n)], l, form, "random_%d_%d" % (l, n))


@pytest.mark.parametrize("form", FORMS)
def test_reference_cell_proof_vectors(kzg, form, golden, blob_loader, oracle_settings):
    """anchor B: every valid compute_cells_and_kzg_proofs vector, byte for byte, through data_availability (bit-reversed)"""
    L = O.lib()
    mono = (O.G1 * 4096)()
    for i in range(4096):
        L.og1_from_affine(C.byref(mono[i]), C.byref(oracle_settings.g1_monomial[i]))
    fs = kzg.FFTSettings(13)
    try:
        w4096 = _root(fs, 4096)
        cases = [c for c in golden["compute_cells_and_kzg_proofs"] if c["output"] is not None]
        assert len(cases) == 7
        polys = []
        for case in cases:
            blob = blob_loader(case["blob"])
            ev = [int.from_bytes(blob[32 * i: 32 * i + 32], "big") for i in range(4096)]
            polys.append(M.ifft([ev[M.brev(i, 12)] for i in range(4096)], w4096))
        with _make(kzg, fs, 8192, 64, form, bytes(mono), 4096) as fk:
            out = fk.data_availability(_fr_bulk([c for p in polys for c in p]), len(polys))
            pts = _points(out, 128 * len(polys))
            for b, case in enumerate(cases):
                comp = b""
                for g in pts[128 * b: 128 * (b + 1)]:
                    buf = C.create_string_buffer(48)
                    L.og1_compress(buf, C.byref(g))
                    comp += buf.raw
                exp = case["output"]
                assert "0x" + comp[:48].hex() == exp["proof0"] and "0x" + comp[-48:].hex() == exp["proof127"], case["name"]
                assert hashlib.sha256(comp).hexdigest() == exp["proofs_sha256"], case["name"]
    finally:
        fs.close()


def test_forms_agree_and_required_table_without_room_is_refused(kzg):
    """anchor C: the two forms give the same group elements; fk20_table=1 with a budget below any table -> NULL"""
    L = O.lib()
    rnd = random.Random(77)
    for l, n in ((1, 64), (8, 256), (16, 16)):
        p = [rnd.randrange(R) for _ in range(n)]
        fs = kzg.FFTSettings((2 * n).bit_length() - 1)
        try:
            outs = []
            for form in FORMS:
                with _make(kzg, fs, 2 * n, l, form) as fk:
                    outs.append(_points(fk.data_availability(_fr_bulk(p), 1, optimized=True), 2 * n // l))
            for j, (a, b) in enumerate(zip(*outs)):
                both_inf = L.og1_is_inf(C.byref(a)) and L.og1_is_inf(C.byref(b))
                assert both_inf or L.og1_equal(C.byref(a), C.byref(b)), (l, n, j)
            with pytest.raises(kzg.KzgAmdError):
                kzg.FK20Settings(fs, _setup(n), n, 2 * n, l, kzg.make_config(table_budget_gb=1e-6, tuning={"fk20_table": 1}))
            # by budget (-1): the same tiny budget falls back to the direct form
            with kzg.FK20Settings(fs, _setup(n), n, 2 * n, l, kzg.make_config(table_budget_gb=1e-6)) as fk:
                assert fk.info()[2] == 1
        finally:
            fs.close()


@pytest.mark.parametrize("form", FORMS)
def test_batches_and_special_polynomials(kzg, form):
    """npoly = 1, 3, 17 in one call == the single calls; the zero and a constant polynomial -> the identity everywhere;
    X^(n-1); 1 + X^(n/2), whose transformed coefficients contain zeros"""
    L = O.lib()
    n, l = 128, 4
    k2 = 2 * n // l
    rnd = random.Random(5)
    zero, const = [0] * n, [12345] + [0] * (n - 1)
    top = [0] * (n - 1) + [1]
    sparse = [1] + [0] * (n - 1)
    sparse[n // 2] = 1
    polys = [zero, const, top, sparse] + [[rnd.randrange(R) for _ in range(n)] for _ in range(13)]
    fs = kzg.FFTSettings(8)
    try:
        with _make(kzg, fs, 2 * n, l, form) as fk:
            single = [_points(fk.data_availability(_fr_bulk(p), 1, optimized=True), k2) for p in polys]
            for i in (0, 1):
                assert all(L.og1_is_inf(C.byref(g)) for g in single[i]), i
            for i in (2, 3, 4):
                _assert_points(single[i], _expected(("special", i), _closed(fs, polys[i], l)), "special %d" % i)
            for npoly in (1, 3, 17):
                flat = [c for p in polys[:npoly] for c in p]
                got = _points(fk.data_availability(_fr_bulk(flat), npoly, optimized=True), npoly * k2)
                for b in range(npoly):
                    for j in range(k2):
                        a, e = got[b * k2 + j], single[b][j]
                        both_inf = L.og1_is_inf(C.byref(a)) and L.og1_is_inf(C.byref(e))
                        assert both_inf or L.og1_equal(C.byref(a), C.byref(e)), (npoly, b, j)
    finally:
        fs.close()


def test_error_codes_in_the_reference_order(kzg):
    L = kzg.lib()
    fs = kzg.FFTSettings(5)
    pts = _setup(32)
    try:
        direct = kzg.make_config(tuning={"fk20_table": 0})

        def new(n2, l, num=32, ntt=fs.handle, mono=pts):
            err = C.c_int(77)
            h = L.kzgamd_fk20_new(ntt, mono, num, n2, l, C.byref(direct), C.byref(err))
            if h:
                L.kzgamd_fk20_free(h)
            return bool(h), err.value

        assert new(64, 1) == (False, 1)
        assert new(64, 3) == (False, 1)      # the width is checked first
        assert new(24, 1) == (False, 2)
        assert new(0, 1) == (False, 2)
        assert new(1, 1) == (False, 3)
        assert new(32, 32) == (False, 4)
        assert new(24, 32) == (False, 2)     # ... and the power of two before the chunk length
        assert new(32, 3) == (False, 5)
        assert new(32, 0) == (False, 5)
        assert new(32, 1, num=14) == (False, 6)
        assert new(32, 1, num=15) == (True, 0)
        assert new(32, 16, num=0) == (True, 0)  # k = 1: no setup point is read
        # fk20_table is read out of the tuning string by this entry point; the other keys go to the library's table
        for tuning, want_ok in (("fk20_table=2", False), ("fk20_table=", False), ("fk20_table=0;nonsense=1", False),
                                ("combine=0;fk20_table=0,g1_wide_max=4096", True), ("fk20_table=-1", True)):
            cfg = kzg.make_config(table_budget_gb=0.1, tuning=tuning)
            e = C.c_int(77)
            h = L.kzgamd_fk20_new(fs.handle, pts, 32, 32, 1, C.byref(cfg), C.byref(e))
            assert bool(h) == want_ok and (e.value == 0) == want_ok, (tuning, e.value)
            if h:
                L.kzgamd_fk20_free(h)
        assert "fk20_table" not in kzg.tuning_keys()
        with pytest.raises(kzg.KzgAmdError):
            kzg.FFTSettings(5, kzg.make_config(tuning="fk20_table=0"))  # not a key of any other handle type
        ok, err = new(32, 1, ntt=None)
        assert not ok and err < 0
        ok, err = new(32, 1, mono=None)
        assert not ok and err < 0
        for code, msg in ((1, "max width"), (2, "n2 must be a power of two"), (4, "chunk_len must be greater"), (5, "chunk_len must be a power")):
            assert msg in kzg.FK20_ERRORS[code]
        with pytest.raises(kzg.KzgAmdError, match="n2 must be a power of two"):
            kzg.FK20Settings(fs, pts, 32, 24, 1)
        with kzg.FK20Settings(fs, pts, 32, 32, 2, kzg.make_config(tuning={"fk20_table": 0})) as fk:
            p = _fr_bulk(list(range(1, 17)))
            out = (kzg.BlstP1 * 16)()
            sentinel = bytes(out)
            assert L.kzgamd_fk20_da(fk.handle, out, p, 8, 1, 0) == 3      # n != n2 / 2
            assert L.kzgamd_fk20_da(fk.handle, out, p, 32, 1, 0) == 3
            assert L.kzgamd_fk20_da(fk.handle, None, p, 16, 1, 0) == -1
            assert L.kzgamd_fk20_da(fk.handle, out, None, 16, 1, 0) == -1
            assert L.kzgamd_fk20_da(fk.handle, out, p, 16, 0, 0) == 0     # npoly = 0: ok, nothing written
            assert L.kzgamd_fk20_da(fk.handle, None, None, 16, 0, 0) == 0
            assert bytes(out) == sentinel
            assert L.kzgamd_fk20_da(fk.handle, out, p, 16, 1, 0) == 0
            assert bytes(out) != sentinel
    finally:
        fs.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", ["single", "multi"])
def test_bench_shapes_at_every_position(kzg, form, shape):
    """bench_fk_single_da (n2 = 2^14, all coefficients one random u64, scale 14) and bench_fk_multi_da (n = 2^14,
    chunk_len 16, scale 15) of the reference (kzg-bench/src/benches/fk20.rs): anchor A at all positions"""
    rnd = random.Random(14)
    if shape == "single":
        scale, n, l = 14, 1 << 13, 1
        p = [rnd.getrandbits(64)] * n
    else:
        scale, n, l = 15, 1 << 14, 16
        p = [rnd.getrandbits(64) for _ in range(n)]
    _check_case(kzg, scale, p, l, form, "bench_" + shape, orders=(True,))


def test_lifecycle_returns_hbm_and_threads_share_handles(kzg):
    """20 x (create, use, free) leaves the free HBM where it was; two threads on one FK20 handle while a third calls
    fft_g1 on the NTT handle under it, every result checked"""
    import torch

    L = O.lib()
    n, l = 256, 4
    k2 = 2 * n // l
    rnd = random.Random(8)
    polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
    fs = kzg.FFTSettings(9)
    try:
        exps = [_expected(("life", i), _closed(fs, polys[i], l)) for i in range(3)]

        def cycle(form):
            with _make(kzg, fs, 2 * n, l, form) as fk:
                _assert_points(_points(fk.data_availability(_fr_bulk(polys[0]), 1, optimized=True), k2), exps[0], "cycle")

        cycle("direct")
        cycle("table")
        fs.fft_g1(_setup(64), 64)  # the NTT handle's own staging, allocated once
        torch.cuda.synchronize()
        base, _ = torch.cuda.mem_get_info(0)
        deltas = []
        for i in range(20):
            cycle("table" if i % 4 == 3 else "direct")
            torch.cuda.synchronize()
            free, _ = torch.cuda.mem_get_info(0)
            deltas.append((base - free) / (1 << 20))
            assert base - free <= (1 << 20), deltas
        print("fk20 lifecycle: HBM delta MB per cycle:", ["%.2f" % d for d in deltas])

        # threads
        g_in = _setup(64)
        ofs = O.FFTSettings()
        assert L.offt_settings_new(C.byref(ofs), 9) == 0
        gin = (O.G1 * 64)()
        C.memmove(gin, g_in, 64 * 144)
        gexp = (O.G1 * 64)()
        assert L.offt_g1(C.byref(ofs), gexp, gin, 64, 0) == 0
        L.offt_settings_free(C.byref(ofs))
        failures = []
        with _make(kzg, fs, 2 * n, l, "direct") as fk:
            def prover(t):
                try:
                    for it in range(6):
                        i = (t + it) % 3
                        if it % 2:
                            flat = [c for p in polys for c in p]
                            got = _points(fk.data_availability(_fr_bulk(flat), 3, optimized=True), 3 * k2)
                            for b in range(3):
                                _assert_points(got[b * k2: (b + 1) * k2], exps[b], "thread batch")
                        else:
                            _assert_points(_points(fk.data_availability(_fr_bulk(polys[i]), 1, optimized=True), k2), exps[i], "thread")
                except Exception as e:  # noqa: BLE001
                    failures.append((t, repr(e)))

            def transformer():
                try:
                    for _ in range(12):
                        got = _points(fs.fft_g1(g_in, 64), 64)
                        for j in range(64):
                            assert L.og1_equal(C.byref(got[j]), C.byref(gexp[j])), j
                except Exception as e:  # noqa: BLE001
                    failures.append(("fft_g1", repr(e)))

            ts = [threading.Thread(target=prover, args=(t,)) for t in range(2)] + [threading.Thread(target=transformer)]
            for th in ts:
                th.start()
            for th in ts:
                th.join()
        assert failures == []
    finally:
        fs.close()
