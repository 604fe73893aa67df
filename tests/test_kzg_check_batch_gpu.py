"""Batched KZG proof checking on the GPU (kzgamd_kzg_check_batch / _check_batch_g1 / kzgamd_kzg_batch_challenge): any
number of (commitment, proof, x, n values) tuples under one pairing.

Anchors, none of them the code under test:
  A. the two G1 sides against the closed form with the known secret (tests/kzg_batch_model.py, pinned on the CPU by
     tests/test_kzg_batch_model_cpu.py): the supplied points are [c_t]G and [q_t]G, so L = [l]G and P = [p]G by the CPU
     oracle's scalar multiplication, the identity checked explicitly — for valid tuples and for corrupted values alike;
  B. verdicts: all valid, exactly one corrupted value / proof / commitment at tuple 0, at the wave edge and at the end,
     ok_each against the per-tuple call;
  C. why the weights matter: errors that cancel unweighted;
  D. the challenge against hashlib, every code, points off the curve and outside G1, empty calls, a handle without G2;
  E. two threads with different n on one handle, and the HBM a handle gives back.
Small handles (FFTSettings(4..7), at most 80 setup points, no wide table)."""
import ctypes as C
import random
import threading

import pytest

import g1_encodings as E
import kzg_batch_model as B
import kzg_model as M
import oracle_ffi as O
from test_fk20_gpu import _fr_bulk, _points, _root
from test_kzg_gpu import _assert_scalars, _expected_point, _handle

pytestmark = pytest.mark.gpu
R = M.R
MB = 1 << 20
NUM_G1 = 80
COUNTS = (1, 2, 63, 64, 65, 257)
ZERO_POINT = bytes(144)

_pool_cache = {}


def _point_bytes(v):
    e = _expected_point(v)
    return ZERO_POINT if e is None else bytes(e)


def _rescale(pt, lam):
    """another Jacobian form of the same point: (X lam^2, Y lam^3, Z lam)"""
    L = O.lib()
    g = O.G1()
    C.memmove(C.byref(g), pt, 144)
    l1 = O.fp_from_int(lam)
    l2, l3 = O.Fp(), O.Fp()
    L.ofp_mul(C.byref(l2), C.byref(l1), C.byref(l1))
    L.ofp_mul(C.byref(l3), C.byref(l2), C.byref(l1))
    out = O.G1()
    L.ofp_mul(C.byref(out.x), C.byref(g.x), C.byref(l2))
    L.ofp_mul(C.byref(out.y), C.byref(g.y), C.byref(l3))
    L.ofp_mul(C.byref(out.z), C.byref(g.z), C.byref(l1))
    assert L.og1_is_inf(C.byref(g)) or L.og1_equal(C.byref(out), C.byref(g))
    return bytes(out)


def _pool(n, w):
    """257 valid tuples for cosets of n values, computed once: scalars (c, q, x, ys), the points' bytes, and per tuple the
    model's terms for the valid values and for corrupted ones.  Among them: a polynomial no longer than n (identity
    proof), the zero polynomial (identity commitment), a repeated tuple, x in {1, R - 1, a root of the coset's own
    order}, and points in Jacobian form with Z != 1."""
    if n in _pool_cache:
        return _pool_cache[n]
    rnd = random.Random(2000 + n)
    polys = [[rnd.randrange(R) for _ in range(n + 5)], [rnd.randrange(R) for _ in range(min(2 * n + 1, NUM_G1))],
             [rnd.randrange(R) for _ in range(n)], [0] * (n + 2)]
    cs = [M.commitment_scalar(p) for p in polys]
    tuples, com, prf = [], [], []
    for t in range(max(COUNTS)):
        if t == 5:  # the tuple before it, again
            tuples.append(tuples[4])
            com.append(com[4])
            prf.append(prf[4])
            continue
        k = t % 4
        x = {0: 1, 1: R - 1, 2: w}.get(t, rnd.randrange(1, R))
        q = M.proof_scalar(polys[k], x, n)
        tuples.append((cs[k], q, x, M.coset_values(polys[k], x, n, w)))
        c_pt, q_pt = _point_bytes(cs[k]), _point_bytes(q)
        if t % 7 == 3 or t in (0, 2):
            c_pt, q_pt = _rescale(c_pt, rnd.randrange(2, O.P)), _rescale(q_pt, rnd.randrange(2, O.P))
        com.append(c_pt)
        prf.append(q_pt)
    assert tuples[2][1] == 0 and tuples[3][0] == 0 and tuples[3][1] == 0  # identities are among the points
    bad_ys = []
    for c, q, x, ys in tuples:
        v = list(ys)
        v[rnd.randrange(n)] = rnd.randrange(R)
        bad_ys.append(v)
    pool = {
        "tuples": tuples, "com": com, "prf": prf, "bad_ys": bad_ys,
        "terms": [B.tuple_terms(*t, n=n, w=w) for t in tuples],
        "bad_terms": [B.tuple_terms(c, q, x, v, n=n, w=w) for (c, q, x, _), v in zip(tuples, bad_ys)],
    }
    _pool_cache[n] = pool
    return pool


def _buffers(pool, count, bad=()):
    """(commitments, proofs, xs, ys) of the first `count` tuples as the library takes them; the values of the tuples in
    `bad` corrupted"""
    ys = [v for t in range(count) for v in (pool["bad_ys"][t] if t in bad else pool["tuples"][t][3])]
    return (b"".join(pool["com"][:count]), b"".join(pool["prf"][:count]), _fr_bulk([t[2] for t in pool["tuples"][:count]]),
            _fr_bulk(ys))


def _terms(pool, count, bad=()):
    return [pool["bad_terms"][t] if t in bad else pool["terms"][t] for t in range(count)]


# ---------------------------------------------------------------- A: the G1 sides against the model
@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_g1_sides_equal_the_model(kzg, n):
    rnd = random.Random(n)
    fs = kzg.FFTSettings(7)
    try:
        w = _root(fs, n) if n > 1 else 1
        pool = _pool(n, w)
        s_n = pow(M.SECRET, n, R)
        with _handle(kzg, fs, NUM_G1) as kz:  # no G2: the G1 sides need none
            for count in COUNTS:
                for bad in ((), tuple(sorted({0, count // 2, count - 1}))):
                    com, prf, xs, ys = _buffers(pool, count, bad)
                    r = rnd.randrange(R)
                    out = kz.check_batch_g1(com, prf, xs, ys, n, count, r=_fr_bulk([r]))
                    l, p = B.combine(_terms(pool, count, bad), r)
                    assert (l == s_n * p % R) == (not bad)
                    _assert_scalars(_points(out, 2), [l, p], "n=%d count=%d bad=%s" % (n, count, bad))
            # the derived weights: r = None hashes these very bytes
            com, prf, xs, ys = _buffers(pool, 65)
            r = B.challenge(com, prf, bytes(xs), bytes(ys), n, 65)
            out = kz.check_batch_g1(com, prf, xs, ys, n, 65)
            _assert_scalars(_points(out, 2), list(B.combine(_terms(pool, 65), r)), "derived r, n=%d" % n)
    finally:
        fs.close()


# ---------------------------------------------------------------- B: verdicts
@pytest.mark.parametrize("n", [1, 8])
def test_verdicts_and_ok_each(kzg, n):
    fs = kzg.FFTSettings(4)
    try:
        w = _root(fs, n) if n > 1 else 1
        pool = _pool(n, w)
        count = 65
        with _handle(kzg, fs, NUM_G1, n + 1) as kz:
            com, prf, xs, ys = _buffers(pool, count)
            assert kz.check_batch(com, prf, xs, ys, n, count) is True
            assert kz.check_batch(com, prf, xs, ys, n, count, each=True) == (True, [True] * count)
            assert kz.check(com, prf, xs, ys, n, count) == [True] * count
            other = _point_bytes(12345)
            for at in (0, 63, 64):  # the first tuple, the last lane of a wave and the first of the next: the last tuple
                for what in ("value", "proof", "commitment"):
                    c2, p2, y2 = com, prf, ys
                    if what == "value":
                        _, _, _, y2 = _buffers(pool, count, (at,))
                    elif what == "proof":
                        p2 = prf[:144 * at] + other + prf[144 * (at + 1):]
                    else:
                        c2 = com[:144 * at] + other + com[144 * (at + 1):]
                    assert kz.check_batch(c2, p2, xs, y2, n, count) is False, (what, at)
            # ok_each is the per-tuple call's answer
            _, _, _, y2 = _buffers(pool, count, (1, 63))
            p2 = prf[:144 * 64] + other
            verdict, each = kz.check_batch(com, p2, xs, y2, n, count, each=True)
            want = kz.check(com, p2, xs, y2, n, count)
            assert verdict is False and each == want == [t not in (1, 63, 64) for t in range(count)]
    finally:
        fs.close()


# ---------------------------------------------------------------- C: why the weights matter
def test_errors_that_cancel_unweighted_are_caught_by_the_weights(kzg):
    rnd = random.Random(31)
    fs = kzg.FFTSettings(4)
    try:
        with _handle(kzg, fs, 16, 2) as kz:
            p = [rnd.randrange(R) for _ in range(9)]
            d = rnd.randrange(1, R)
            x = [rnd.randrange(R) for _ in range(2)]
            y = [M.evaluate(p, v) for v in x]
            com = _point_bytes(M.commitment_scalar(p)) * 2
            prf = b"".join(_point_bytes(M.proof_scalar(p, v, 1)) for v in x)
            xs = _fr_bulk(x)
            good, bad = _fr_bulk(y), _fr_bulk([(y[0] + d) % R, (y[1] - d) % R])
            assert kz.check(com, prf, xs, bad, 1, 2) == [False, False]
            assert kz.check_batch(com, prf, xs, bad, 1, 2, r=_fr_bulk([1])) is True    # the two errors cancel in the plain sum
            assert kz.check_batch(com, prf, xs, bad, 1, 2) is False                    # the derived weights
            assert kz.check_batch(com, prf, xs, bad, 1, 2, r=_fr_bulk([rnd.randrange(2, R)])) is False
            # r = 0 weighs tuple 0 alone: what a caller-supplied r means
            half = _fr_bulk([y[0], (y[1] - d) % R])
            assert kz.check_batch(com, prf, xs, half, 1, 2, r=_fr_bulk([0])) is True
            assert kz.check_batch(com, prf, xs, bad, 1, 2, r=_fr_bulk([0])) is False
            assert kz.check_batch(com, prf, xs, good, 1, 2) is True
    finally:
        fs.close()


# ---------------------------------------------------------------- D: challenge, codes, bad points, empty calls
def test_challenge_equals_the_model_and_none_means_the_derived_value(kzg):
    fs = kzg.FFTSettings(4)
    try:
        n, count = 8, 5
        pool = _pool(n, _root(fs, n))
        with _handle(kzg, fs, NUM_G1, n + 1) as kz:
            for bad in ((), (3,)):
                com, prf, xs, ys = _buffers(pool, count, bad)
                r = kzg.batch_challenge(com, prf, xs, ys, n, count)
                want = B.challenge(com, prf, bytes(xs), bytes(ys), n, count)
                assert int.from_bytes(bytes(r), "little") == (want << 256) % R
                derived, given = kz.check_batch_g1(com, prf, xs, ys, n, count), kz.check_batch_g1(com, prf, xs, ys, n, count, r=r)
                _assert_scalars(_points(derived, 2), list(B.combine(_terms(pool, count, bad), want)), "derived")
                _assert_scalars(_points(given, 2), list(B.combine(_terms(pool, count, bad), want)), "given")
                assert kz.check_batch(com, prf, xs, ys, n, count) == kz.check_batch(com, prf, xs, ys, n, count, r=r) == (not bad)
    finally:
        fs.close()


def _jacobian(affine):
    """blst_p1 bytes of an affine point given as Python integers (x, y), Z = 1"""
    g, a = O.G1(), O.G1Affine()
    a.x, a.y = O.fp_from_int(affine[0]), O.fp_from_int(affine[1])
    O.lib().og1_from_affine(C.byref(g), C.byref(a))
    return bytes(g)


def test_codes_bad_points_and_empty_calls(kzg):
    L = kzg.lib()
    LO = O.lib()
    fs = kzg.FFTSettings(3)
    try:
        n = 4
        pool = _pool(n, _root(fs, n))
        com, prf, xs, ys = _buffers(pool, 3)
        ok, each = C.c_bool(False), (C.c_bool * 3)()
        out = (kzg.BlstP1 * 2)()
        sentinel = bytes(range(144)) * 2
        C.memmove(out, sentinel, 288)
        zero_x = _fr_bulk([5, 0, 7])
        with _handle(kzg, fs, NUM_G1, 5) as kz:
            h = kz.handle

            def batch(n_=n, count=3, ok_=C.byref(ok), c=com, p=prf, x=xs, y=ys, r=None):
                return L.kzgamd_kzg_check_batch(h, ok_, each, c, p, x, y, n_, count, r)

            def sides(n_=n, count=3, out_=out, c=com, p=prf, x=xs, y=ys):
                return L.kzgamd_kzg_check_batch_g1(h, out_, c, p, x, y, n_, count, None)

            assert batch() == 0 and ok.value is True and list(each) == [True] * 3
            # 3, 4, 6, 1, 5 in kzgamd_kzg_check's order
            ok.value = False
            assert batch(0) == 3 and batch(3) == 3 and sides(0) == 3 and sides(6) == 3
            assert batch(16) == 4 and sides(16) == 4
            assert batch(8) == 6          # num_g2 = 5 <= 8
            assert sides(8, x=_fr_bulk([3, 5, 7]), y=_fr_bulk([0] * 24)) == 0   # ... which the G1 sides do not need
            assert batch(x=zero_x) == 5 and sides(x=zero_x) == 5
            assert batch(1, x=zero_x) == 0     # x = 0 is a point like any other for n = 1 (the verdict: whatever it is)
            # NULL arguments
            assert batch(ok_=None) == -1 and batch(c=None) == -1 and batch(p=None) == -1 and batch(x=None) == -1 and batch(y=None) == -1
            assert sides(out_=None) == -1 and sides(c=None) == -1 and sides(y=None) == -1
            assert L.kzgamd_kzg_check_batch(None, C.byref(ok), None, com, prf, xs, ys, n, 3, None) == -1
            # count = 0: ok, true; two identities
            ok.value = False
            assert batch(count=0, c=None, p=None, x=None, y=None) == 0 and ok.value is True
            assert sides(count=0, c=None, p=None, x=None, y=None) == 0 and bytes(out) == bytes(288)
            assert batch(count=0, ok_=None) == -1 and sides(count=0, out_=None) == -1   # what is written is required
            # 7: off the curve, and on the curve outside G1 — nothing written
            C.memmove(out, sentinel, 288)
            off = bytearray(pool["com"][1])
            off[0] ^= 1
            outside = []
            for name, enc in E.by_class(2)[:4] + [e for e in E.by_class(2) if e[0].startswith("order 11")][:1]:
                a = O.G1Affine()
                assert LO.og1_uncompress(C.byref(a), enc) and LO.og1_affine_on_curve(C.byref(a)), name
                g = O.G1()
                LO.og1_from_affine(C.byref(g), C.byref(a))
                assert not LO.og1_in_subgroup(C.byref(g)), name
                outside.append((name, _rescale(bytes(g), 3)))
            for name, pt in [("off the curve", bytes(off))] + outside:
                for slot in range(3):
                    for which in ("commitment", "proof"):
                        c2, p2 = com, prf
                        if which == "commitment":
                            c2 = com[:144 * slot] + pt + com[144 * (slot + 1):]
                        else:
                            p2 = prf[:144 * slot] + pt + prf[144 * (slot + 1):]
                        ok.value = True
                        each[:] = [True] * 3
                        assert batch(c=c2, p=p2) == 7, (name, slot, which)
                        assert ok.value is True and list(each) == [True] * 3
                        assert sides(c=c2, p=p2) == 7 and bytes(out) == sentinel, (name, slot, which)
            with pytest.raises(kzg.KzgAmdError, match="not on the curve or not in G1"):
                kz.check_batch(bytes(off) + com[144:], prf, xs, ys, n, 3)
            assert batch() == 0 and ok.value is True   # the handle is as good as before
        with _handle(kzg, fs, 2, 9) as kz:
            assert L.kzgamd_kzg_check_batch(kz.handle, C.byref(ok), None, com, prf, xs, ys, n, 3, None) == 1   # n > num_g1
            assert L.kzgamd_kzg_check_batch_g1(kz.handle, out, com, prf, xs, ys, n, 3, None) == 1
        # a handle without G2: the G1 sides work, the verdict needs the setup
        with _handle(kzg, fs, NUM_G1) as kz:
            got = kz.check_batch_g1(com, prf, xs, ys, n, 3, r=_fr_bulk([987654321]))
            _assert_scalars(_points(got, 2), list(B.combine(_terms(pool, 3), 987654321)), "no G2")
            assert L.kzgamd_kzg_check_batch(kz.handle, C.byref(ok), None, com, prf, xs, ys, n, 3, None) == 6
            with pytest.raises(kzg.KzgAmdError, match="too few G2 points"):
                kz.check_batch(com, prf, xs, ys, n, 3)
    finally:
        fs.close()


# ---------------------------------------------------------------- E: threads and lifecycle
def test_threads_with_different_n_share_a_handle_and_hbm_comes_back(kzg):
    import torch

    fs = kzg.FFTSettings(4)
    try:
        ns = (1, 2, 8)
        pools = {n: _pool(n, _root(fs, n) if n > 1 else 1) for n in ns}
        count = 9

        def cycle():
            with _handle(kzg, fs, NUM_G1, 9) as kz:
                for n in (1, 8):
                    assert kz.check_batch(*_buffers(pools[n], count), n, count) is True

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
        print("kzg check_batch lifecycle: HBM delta MB per cycle:", ["%.2f" % d for d in deltas])

        with _handle(kzg, fs, NUM_G1, 9) as kz:
            good = {n: _buffers(pools[n], count) for n in ns}
            bad = {n: _buffers(pools[n], count, (count - 1,)) for n in ns}
            failures = []

            def work(t):
                try:
                    for it in range(6):
                        n = ns[(t + it) % len(ns)]   # the line table of [s^n]G2 is looked up, or built, under the lock
                        assert kz.check_batch(*good[n], n, count) is True
                        assert kz.check_batch(*bad[n], n, count) is False
                except Exception as e:  # noqa: BLE001
                    failures.append((t, repr(e)))

            ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
            for th in ts:
                th.start()
            for th in ts:
                th.join()
            assert failures == []
    finally:
        fs.close()
