"""Generic polynomial KZG on the GPU (kzgamd_kzg_new / _commit / _open / _check): commit_to_poly, compute_proof_single,
compute_proof_multi, check_proof_single and check_proof_multi of the reference's KZGSettings, batched.

Anchors, none of them the code under test:
  A. the closed form with the known secret (tests/kzg_model.py, pinned on the CPU by tests/test_kzg_model_cpu.py): the
     setup is [s^i]G for the reference's public SECRET, so a commitment must be [p(s)]G and a proof
     [(p(s) - r(s)) / (s^n - x^n)]G — [scalar]G by the CPU oracle, the identity checked explicitly — and every value
     of ys the Python-integer evaluation p(x w^i);
  B. the reference's compute_kzg_proof vectors over the mainnet monomial setup;
  C. the reference's own test programs (kzg-bench/src/tests/kzg_proofs.rs) restated;
  D. batched checks with corrupted tuples, every error code, empty calls, a handle without G2;
  E. lifecycle and threads.
Small handles get no wide table or a small explicit table budget."""
import ctypes as C
import os
import random
import threading

import pytest

import fk20_model as FM
import kzg_model as M
import oracle_ffi as O
from test_fk20_gpu import _fr_bulk, _points, _root, _setup

pytestmark = pytest.mark.gpu
R = M.R
MB = 1 << 20
SETUP_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trusted_setup.txt")

_expected_cache = {}
_g2_cache = {}


def _expected_point(v):
    """[v]G by the oracle (None for zero: the identity), cached per scalar"""
    if v == 0:
        return None
    if v not in _expected_cache:
        L = O.lib()
        g, e = O.G1(), O.G1()
        L.og1_generator(C.byref(g))
        L.og1_mul(C.byref(e), C.byref(g), C.byref(O.fr_from_int(v)))
        _expected_cache[v] = e
    return _expected_cache[v]


def _assert_scalars(got, scalars, what):
    L = O.lib()
    assert len(got) == len(scalars)
    for j, (g, v) in enumerate(zip(got, scalars)):
        e = _expected_point(v)
        if e is None:
            assert L.og1_is_inf(C.byref(g)), (what, j, "expected the identity")
        else:
            assert not L.og1_is_inf(C.byref(g)) and L.og1_equal(C.byref(g), C.byref(e)), (what, j)


def _same_points(a, b, what):
    L = O.lib()
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        both_inf = L.og1_is_inf(C.byref(x)) and L.og1_is_inf(C.byref(y))
        assert both_inf or (not L.og1_is_inf(C.byref(x)) and L.og1_equal(C.byref(x), C.byref(y))), (what, j)


def _fr_ints(arr, count):
    raw = bytes(arr)
    inv = pow(1 << 256, R - 2, R)
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") * inv % R for i in range(count)]


def _g2_setup(kzg, count):
    """[s^i]G2, i < count, as a contiguous blst_p2 array (host arithmetic of the library's pairing code)"""
    have = _g2_cache.setdefault(id(kzg), [])
    g = kzg.p2_generator()
    while len(have) < count:
        have.append(bytes(kzg.p2_mult(g, _fr_bulk([pow(M.SECRET, len(have), R)])[0])))
    arr = (kzg.BlstP2 * count)()
    C.memmove(arr, b"".join(have[:count]), count * C.sizeof(kzg.BlstP2))
    return arr


def _handle(kzg, fs, num_g1, num_g2=0, config=None):
    cfg = config if config is not None else kzg.make_config(no_tables=True)
    return kzg.PolyKZGSettings(fs, _setup(num_g1), num_g1, _g2_setup(kzg, num_g2) if num_g2 else None, num_g2, cfg)


def _values(p, x, n, w):
    """p(x w^i), i < n: directly for small n, through the remainder's transform (pinned equal on the CPU) for large n"""
    if n * len(p) <= 1 << 16:
        return M.coset_values(p, x, n, w)
    _, r = M.long_division(p, n, pow(x, n, R))
    return FM.fft([r[j] * pow(x, j, R) % R for j in range(n)], w)


def _check_open(kz, fs, polys, xs, n, what):
    """one open call for all (polynomial, x) pairs against the closed forms; returns the proofs"""
    ln, npoly, nx = len(polys[0]), len(polys), len(xs)
    w = _root(fs, n) if n > 1 else 1
    proofs, ys = kz.open(_fr_bulk([c for p in polys for c in p]), ln, npoly, _fr_bulk(xs), nx, n)
    pts = _points(proofs, npoly * nx)
    _assert_scalars(pts, [M.proof_scalar(p, x, n) for p in polys for x in xs], what)
    got = _fr_ints(ys, npoly * nx * n)
    want = [v for p in polys for x in xs for v in _values(p, x, n, w)]
    assert got == want, what
    return pts


def _xs(rnd, fs, n):
    return [0, 1, R - 1, _root(fs, n) if n > 1 else 1, rnd.randrange(R)]


# ---------------------------------------------------------------- A: closed form
def test_single_proofs_across_chunk_wave_and_summary_boundaries(kzg):
    rnd = random.Random(1)
    fs = kzg.FFTSettings(4)
    try:
        with _handle(kzg, fs, 2200) as kz:
            num_g1, num_g2, chunk, lane_min = kz.info()
            assert (num_g1, num_g2) == (2200, 0) and chunk >= 1 and lane_min >= 1
            lens = [1, 2, 3, chunk - 1, chunk, chunk + 1, 64 * chunk - 1, 64 * chunk, 64 * chunk + 1, 64 * chunk + chunk + 1,
                    2 * 64 * chunk + chunk + 5]  # the last: three waves of summaries
            assert lens[-1] <= 2200
            for ln in sorted(set(v for v in lens if v >= 1)):
                p = [rnd.randrange(R) for _ in range(ln)]
                _check_open(kz, fs, [p], _xs(rnd, fs, 1), 1, "n=1 len=%d" % ln)
                _assert_scalars(_points(kz.commit(_fr_bulk(p), ln), 1), [M.commitment_scalar(p)], "commit len=%d" % ln)
    finally:
        fs.close()


_line_cache = {}


def _line_points(count):
    """[i + 1]G, i < count, by repeated addition: a setup without a secret, for lengths a known-secret setup would take
    minutes to build — a commitment over it is [sum q_i (i + 1)]G"""
    if _line_cache.get("count", 0) < count:
        L = O.lib()
        g, cur = O.G1(), O.G1()
        L.og1_generator(C.byref(g))
        L.og1_generator(C.byref(cur))
        arr = (O.G1 * count)()
        for i in range(count):
            C.memmove(C.byref(arr[i]), C.byref(cur), 144)
            nxt = O.G1()
            L.og1_add_or_dbl(C.byref(nxt), C.byref(cur), C.byref(g))
            cur = nxt
        _line_cache.update(count=count, pts=arr)
    return _line_cache["pts"]


def test_single_proof_longer_than_a_block_of_wave_summaries(kzg):
    """n = 1 with more than 64 waves of chunks: the carries across waves take more than one block of 64 summaries.  The
    quotient is held to Python long division through its commitment over the points [i + 1]G, the value to evaluation."""
    rnd = random.Random(6)
    fs = kzg.FFTSettings(4)
    try:
        probe = _handle(kzg, fs, 4)
        chunk = probe.info()[2]
        probe.close()
        ln = 64 * 64 * chunk + 3 * chunk + 5
        pts = _line_points(ln - 1)
        p = [rnd.randrange(R) for _ in range(ln)]
        xs = [rnd.randrange(R), R - 1]
        with kzg.PolyKZGSettings(fs, pts, ln - 1, None, 0, kzg.make_config(no_tables=True)) as kz:
            proofs, ys = kz.open(_fr_bulk(p), ln, 1, _fr_bulk(xs), 2, 1)
            want = []
            for x in xs:
                q, r = M.long_division(p, 1, x)
                assert r == [M.evaluate(p, x)]
                want.append(sum(v * (i + 1) for i, v in enumerate(q)) % R)
            _assert_scalars(_points(proofs, 2), want, "long n=1")
            assert _fr_ints(ys, 2) == [M.evaluate(p, x) for x in xs]
    finally:
        fs.close()


@pytest.mark.parametrize("n", [2, 8, 64])
def test_coset_proofs(kzg, n):
    rnd = random.Random(n)
    fs = kzg.FFTSettings(7)
    try:
        with _handle(kzg, fs, 1000) as kz:
            for ln in (n - 1, n, n + 1, 2 * n - 1, 2 * n + 1, 1000):
                p = [rnd.randrange(R) for _ in range(ln)]
                _check_open(kz, fs, [p], _xs(rnd, fs, n), n, "n=%d len=%d" % (n, ln))
    finally:
        fs.close()


def test_both_forms_of_the_quotient_agree_at_the_threshold(kzg):
    """(n, pairs) just below and just above lane_form_min with the same polynomial: the scan form, the lane form"""
    rnd = random.Random(3)
    fs = kzg.FFTSettings(10)
    try:
        with _handle(kzg, fs, 400) as kz:
            lane_min = kz.info()[3]
            n = 1024
            assert lane_min % n == 0 and lane_min // n >= 2
            above = lane_min // n
            p = [rnd.randrange(R) for _ in range(n + 300)]
            xs = [rnd.randrange(R) for _ in range(above - 2)] + [_root(fs, n), R - 1]
            lanes = _check_open(kz, fs, [p], xs, n, "lane form")
            scan = _check_open(kz, fs, [p], xs[:-1], n, "scan form")
            _same_points(lanes[:-1], scan, "forms")
    finally:
        fs.close()


def test_batch_equals_single_calls_and_zero_polynomials(kzg):
    L = O.lib()
    rnd = random.Random(4)
    fs = kzg.FFTSettings(5)
    try:
        with _handle(kzg, fs, 300) as kz:
            for n, ln in ((1, 300), (4, 77)):
                polys = [[rnd.randrange(R) for _ in range(ln)] for _ in range(3)]
                xs = [rnd.randrange(R) for _ in range(5)]
                batch = _check_open(kz, fs, polys, xs, n, "batch n=%d" % n)
                single = []
                for p in polys:
                    for x in xs:
                        pr, _ = kz.open(_fr_bulk(p), ln, 1, _fr_bulk([x]), 1, n)
                        single += _points(pr, 1)
                _same_points(batch, single, "batch against single n=%d" % n)
                _assert_scalars(_points(kz.commit(_fr_bulk([c for p in polys for c in p]), ln, 3), 3),
                                [M.commitment_scalar(p) for p in polys], "commit batch")
                # zero top coefficients, and the all-zero polynomial: identities
                low = [rnd.randrange(R) for _ in range(ln // 2)] + [0] * (ln - ln // 2)
                zero = [0] * ln
                pts = _check_open(kz, fs, [low, zero], xs[:2], n, "zero tops n=%d" % n)
                assert all(L.og1_is_inf(C.byref(g)) for g in pts[2:])
                assert L.og1_is_inf(C.byref(_points(kz.commit(_fr_bulk(zero), ln), 1)[0]))
    finally:
        fs.close()


# ---------------------------------------------------------------- B: the reference's vectors
def test_reference_compute_kzg_proof_vectors(kzg, golden, blob_loader):
    fs = kzg.FFTSettings(12)
    s = kzg.KZGSettings.from_file(SETUP_FILE, kzg.make_config(table_budget_gb=1))
    try:
        mono = (kzg.BlstP1 * 4096).from_address(s.c.g1_values_monomial)
        commitments = {c["blob"]: c["output"] for c in golden["blob_to_kzg_commitment"] if c["output"] is not None}
        w = _root(fs, 4096)
        domain = {1, R - 1}
        assert pow(w, 2048, R) == R - 1
        cases = [c for c in golden["compute_kzg_proof"] if c["output"] is not None and "_blob_2_" in c["name"]]
        cases += [c for c in golden["compute_kzg_proof"] if c["output"] is not None and "_blob_4_" in c["name"]][1:4]
        zs = [int(c["z"], 16) for c in cases]
        assert any(z in domain for z in zs) and any(pow(z, 4096, R) != 1 for z in zs)

        def point(hex48):
            p = kzg.bytes_to_kzg_commitment(bytes.fromhex(hex48[2:]))
            g = O.G1()
            C.memmove(C.byref(g), bytes(p), 144)
            return g

        with kzg.PolyKZGSettings(fs, mono, 4096, None, 0, kzg.make_config(table_budget_gb=1)) as kz:
            coeffs = {}
            for case in cases:
                ref = case["blob"]
                if ref not in coeffs:
                    blob = blob_loader(ref)
                    ev = [int.from_bytes(blob[32 * i: 32 * i + 32], "big") for i in range(4096)]
                    nat = _fr_bulk([ev[FM.brev(i, 12)] for i in range(4096)])
                    coeffs[ref] = fs.fft_fr(nat, 4096, inverse=True)
                    com = _points(kz.commit(coeffs[ref], 4096), 1)
                    _same_points(com, [point(commitments[ref])], "commitment " + ref)
                z = int(case["z"], 16)
                proofs, ys = kz.open(coeffs[ref], 4096, 1, _fr_bulk([z]), 1, 1)
                _same_points(_points(proofs, 1), [point(case["output"][0])], case["name"])
                assert _fr_ints(ys, 1) == [int(case["output"][1], 16)], case["name"]
    finally:
        s.close()
        fs.close()


# ---------------------------------------------------------------- C: the reference's test programs
REF_POLY = [1, 2, 3, 4, 7, 7, 7, 7, 13, 13, 13, 13, 13, 13, 13]


def test_reference_proof_single_and_multi_programs(kzg):
    L = O.lib()
    fs = kzg.FFTSettings(3)
    try:
        # a small explicit table budget: this handle runs the wide-table engine
        with _handle(kzg, fs, 16, 9, kzg.make_config(table_budget_gb=0.1)) as kz:
            p = _fr_bulk(REF_POLY)
            com = kz.commit(p, 15)
            _assert_scalars(_points(com, 1), [M.commitment_scalar(REF_POLY)], "commit")
            # proof_single: x = 25
            proof, ys = kz.open(p, 15, 1, _fr_bulk([25]), 1, 1)
            y = M.evaluate(REF_POLY, 25)
            assert _fr_ints(ys, 1) == [y]
            assert kz.check(com, proof, _fr_bulk([25]), _fr_bulk([y]), 1, 1) == [True]
            assert kz.check(com, proof, _fr_bulk([25]), _fr_bulk([(y + 1) % R]), 1, 1) == [False]
            # proof_multi: x = 5431, coset of 8
            proof, ys = kz.open(p, 15, 1, _fr_bulk([5431]), 1, 8)
            vals = M.coset_values(REF_POLY, 5431, 8, _root(fs, 8))
            assert _fr_ints(ys, 8) == vals
            assert kz.check(com, proof, _fr_bulk([5431]), _fr_bulk(vals), 8, 1) == [True]
            bad = list(vals)
            bad[4] = (bad[4] + 1) % R
            assert kz.check(com, proof, _fr_bulk([5431]), _fr_bulk(bad), 8, 1) == [False]
            # commit_to_nil_poly, commit_to_too_long_poly_returns_err
            assert L.og1_is_inf(C.byref(_points(kz.commit(_fr_bulk([]), 0), 1)[0]))
            with pytest.raises(kzg.KzgAmdError, match="Polynomial is longer than secret g1"):
                kz.commit(_fr_bulk([1] * 17), 17)
    finally:
        fs.close()


# ---------------------------------------------------------------- D: batched checks, error codes, empty calls
@pytest.mark.parametrize("n", [1, 8])
def test_check_batch_flags_exactly_the_corrupted_tuples(kzg, n):
    rnd = random.Random(20 + n)
    fs = kzg.FFTSettings(4)
    try:
        with _handle(kzg, fs, 40, n + 1) as kz:
            w = _root(fs, n) if n > 1 else 1
            polys = [[rnd.randrange(R) for _ in range(33)] for _ in range(6)]
            xs = [rnd.randrange(1, R) for _ in range(6)]
            coms, proofs, vals = b"", b"", []
            for p, x in zip(polys, xs):
                coms += bytes(kz.commit(_fr_bulk(p), 33))[:144]
                pr, _ = kz.open(_fr_bulk(p), 33, 1, _fr_bulk([x]), 1, n, want_ys=False)
                proofs += bytes(pr)[:144]
                vals += M.coset_values(p, x, n, w)
            assert kz.check(coms, proofs, _fr_bulk(xs), _fr_bulk(vals), n, 6) == [True] * 6
            bad_vals = list(vals)
            bad_vals[1 * n + n // 2] = (bad_vals[1 * n + n // 2] + 1) % R          # 2nd tuple: a wrong value
            bad_proofs = proofs[:4 * 144] + proofs[0:144] + proofs[5 * 144:]         # 5th tuple: another tuple's proof
            assert kz.check(coms, bad_proofs, _fr_bulk(xs), _fr_bulk(bad_vals), n, 6) == [True, False, True, True, False, True]
    finally:
        fs.close()


def test_error_codes_and_empty_calls(kzg):
    L = kzg.lib()
    fs = kzg.FFTSettings(3)
    try:
        pts, g2 = _setup(8), _g2_setup(kzg, 5)
        none = kzg.make_config(no_tables=True)

        def new(num_g1=8, ntt=fs.handle, mono=pts, g2m=g2, num_g2=5, cfg=none):
            err = C.c_int(77)
            h = L.kzgamd_kzg_new(ntt, mono, num_g1, g2m, num_g2, C.byref(cfg) if cfg is not None else None, C.byref(err))
            if h:
                L.kzgamd_kzg_free(h)
            return bool(h), err.value

        assert new() == (True, 0)
        assert new(num_g1=0) == (False, 1)
        assert new(num_g1=0, ntt=None) == (False, 1)   # the reference's check first
        assert new(ntt=None) == (False, -1)
        assert new(mono=None) == (False, -1)
        assert new(g2m=None) == (False, -1)            # num_g2 != 0 without points
        assert new(g2m=None, num_g2=0) == (True, 0)
        assert new(cfg=kzg.make_config(no_tables=True, tuning="nonsense=1")) == (False, -2)
        with pytest.raises(kzg.KzgAmdError, match="no G1 points"):
            kzg.PolyKZGSettings(fs, pts, 0)

        p = _fr_bulk(list(range(1, 13)))
        x = _fr_bulk([5, 7])
        out = (kzg.BlstP1 * 4)()
        sentinel = bytes(out)
        ok = (C.c_bool * 4)()
        with kzg.PolyKZGSettings(fs, pts, 8, g2, 5, none) as kz:
            h = kz.handle
            assert kz.info()[:2] == (8, 5)
            # commit
            assert L.kzgamd_kzg_commit(h, out, p, 9, 1) == 1
            assert L.kzgamd_kzg_commit(h, None, p, 8, 1) == -1
            assert L.kzgamd_kzg_commit(h, out, None, 8, 1) == -1
            assert L.kzgamd_kzg_commit(h, None, None, 8, 0) == 0       # npoly = 0: ok, nothing written
            assert bytes(out) == sentinel
            assert L.kzgamd_kzg_commit(h, out, p, 8, 1) == 0 and bytes(out) != sentinel
            # open: 2 (empty), 3 (n), 1 (quotient longer than the setup), 4 (ys beyond the max width), in that order
            assert L.kzgamd_kzg_open(h, out, None, p, 0, 1, x, 1, 3) == 2
            assert L.kzgamd_kzg_open(h, out, None, p, 12, 1, x, 1, 0) == 3
            assert L.kzgamd_kzg_open(h, out, None, p, 12, 1, x, 1, 3) == 3
            assert L.kzgamd_kzg_open(h, out, None, p, 12, 1, x, 1, 2) == 1
            ys = (kzg.BlstFr * 32)()
            assert L.kzgamd_kzg_open(h, out, ys, p, 12, 1, x, 1, 16) == 4
            assert L.kzgamd_kzg_open(h, out, None, p, 12, 1, x, 1, 16) == 0   # without ys the width does not matter
            assert L.kzgamd_kzg_open(h, None, None, p, 8, 1, x, 1, 1) == -1
            assert L.kzgamd_kzg_open(h, out, None, None, 8, 1, x, 1, 1) == -1
            assert L.kzgamd_kzg_open(h, out, None, p, 8, 1, None, 1, 1) == -1
            out = (kzg.BlstP1 * 4)()
            assert L.kzgamd_kzg_open(h, None, None, None, 8, 0, x, 2, 1) == 0  # npoly = 0
            assert L.kzgamd_kzg_open(h, out, None, p, 8, 1, None, 0, 1) == 0   # nx = 0
            assert bytes(out) == sentinel
            with pytest.raises(kzg.KzgAmdError, match="Polynomial must not be empty"):
                kz.open(_fr_bulk([]), 0, 1, x, 1, 1)
            with pytest.raises(kzg.KzgAmdError, match="n must be a power of two"):
                kz.open(p, 8, 1, x, 1, 6)
            # check: 3, 4, 6, 1, 5 in that order
            com = kz.commit(p, 8)
            proof, vals = kz.open(p, 8, 1, x, 1, 4)
            assert kz.check(com, proof, x, vals, 4, 1) == [True]
            assert L.kzgamd_kzg_check(h, ok, com, proof, x, vals, 0, 1) == 3
            assert L.kzgamd_kzg_check(h, ok, com, proof, x, vals, 3, 1) == 3
            assert L.kzgamd_kzg_check(h, ok, com, proof, x, vals, 16, 1) == 4
            assert L.kzgamd_kzg_check(h, ok, com, proof, x, vals, 8, 1) == 6      # num_g2 = 5 <= 8
            assert L.kzgamd_kzg_check(h, ok, com, proof, _fr_bulk([0]), vals, 4, 1) == 5
            assert L.kzgamd_kzg_check(h, ok, com, proof, _fr_bulk([0]), vals, 1, 1) == 0   # x = 0 is a point like any other for n = 1
            assert L.kzgamd_kzg_check(h, None, com, proof, x, vals, 4, 1) == -1
            assert L.kzgamd_kzg_check(h, None, None, None, None, None, 4, 0) == 0   # count = 0
        with kzg.PolyKZGSettings(fs, pts, 2, _g2_setup(kzg, 9), 9, none) as kz:
            assert L.kzgamd_kzg_check(kz.handle, ok, out, out, x, _fr_bulk([0] * 8), 4, 1) == 1   # n > num_g1
        # a handle without G2 proves, and refuses to check
        with kzg.PolyKZGSettings(fs, pts, 8, None, 0, none) as kz:
            assert kz.info()[:2] == (8, 0)
            com = kz.commit(p, 8)
            proof, vals = kz.open(p, 8, 1, x, 1, 1)
            assert L.kzgamd_kzg_check(kz.handle, ok, com, proof, x, vals, 1, 1) == 6
            with pytest.raises(kzg.KzgAmdError, match="too few G2 points"):
                kz.check(com, proof, x, vals, 1, 1)
        for code, msg in ((1, "longer than secret g1"), (2, "must not be empty"), (3, "power of two")):
            assert msg in kzg.KZG_ERRORS[code]
    finally:
        fs.close()


# ---------------------------------------------------------------- E: lifecycle and threads
def test_lifecycle_returns_hbm_and_threads_share_a_handle(kzg):
    import torch

    rnd = random.Random(9)
    fs = kzg.FFTSettings(5)
    try:
        polys = [[rnd.randrange(R) for _ in range(200)] for _ in range(3)]
        xs = [rnd.randrange(1, R) for _ in range(4)]
        flat = _fr_bulk([c for p in polys for c in p])

        def cycle():
            with _handle(kzg, fs, 200, 9) as kz:
                _check_open(kz, fs, polys[:1], xs[:2], 8, "cycle")

        cycle()
        torch.cuda.synchronize()
        base, _ = torch.cuda.mem_get_info(0)
        deltas = []
        for _ in range(10):
            cycle()
            torch.cuda.synchronize()
            free, _ = torch.cuda.mem_get_info(0)
            deltas.append((base - free) / MB)
            assert base - free <= 8 * MB, deltas
        print("kzg lifecycle: HBM delta MB per cycle:", ["%.2f" % d for d in deltas])

        with _handle(kzg, fs, 200, 9) as kz:
            coms = bytes(kz.commit(flat, 200, 3))
            want = {}
            for n in (1, 8):
                proofs, ys = kz.open(flat, 200, 3, _fr_bulk(xs), 4, n)
                want[n] = (bytes(proofs), bytes(ys))
                _check_open(kz, fs, polys, xs, n, "single thread n=%d" % n)
            # the tuples (polynomial 0, x_k) for check
            com4 = coms[:144] * 4
            failures = []

            def work(t):
                try:
                    for it in range(4):
                        n = (1, 8)[(t + it) % 2]
                        _same_points(_points(kz.commit(flat, 200, 3), 3), _points(coms, 3), "thread commit")
                        proofs, ys = kz.open(flat, 200, 3, _fr_bulk(xs), 4, n)
                        _same_points(_points(proofs, 12), _points(want[n][0], 12), "thread open")
                        assert bytes(ys) == want[n][1]
                        assert kz.check(com4, want[n][0][:4 * 144], _fr_bulk(xs), want[n][1][:4 * n * 32], n, 4) == [True] * 4
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
