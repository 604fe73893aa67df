"""kzgamd_kzg_check, and the ok_each of a failing kzgamd_kzg_check_batch, with their pairings on the GPU (tuning key
pairing_gpu_min = 1: one wave per tuple, pairing.hip) against the same calls with the host loop (pairing_gpu_min = 0):
two handles over the same setup, the verdicts tuple by tuple.

n in {1, 2, 16}, count in {1, 5, 70}; valid tuples (among them identity proofs and commitments, a repeated tuple, points
with Z != 1: the pool of tests/test_kzg_check_batch_gpu.py), a wrong y, a wrong proof, a wrong commitment, proof =
identity, a proof and a commitment on the curve outside G1 (n = 1 and n = 16: the GLV multiplication and the
rearrangement of the GPU form only hold in G1, such tuples must reach the host loop) and a point off the curve; the
error codes for x = 0 and n > width are unchanged.  Setups of 64 G1 points, no wide table."""
import ctypes as C

import pytest

import g1_encodings as E
import oracle_ffi as O
from test_fk20_gpu import _fr_bulk, _root
from test_kzg_check_batch_gpu import ZERO_POINT, _buffers, _point_bytes, _pool, _rescale
from test_kzg_gpu import _handle

pytestmark = pytest.mark.gpu
NUM_G1 = 64
COUNTS = (1, 5, 70)


def _two_handles(kzg, fs, n):
    gpu = _handle(kzg, fs, NUM_G1, n + 1, config=kzg.make_config(no_tables=True, tuning="pairing_gpu_min=1"))
    host = _handle(kzg, fs, NUM_G1, n + 1, config=kzg.make_config(no_tables=True, tuning="pairing_gpu_min=0"))
    return gpu, host


def _swap(buf, at, pt):
    return buf[:144 * at] + pt + buf[144 * (at + 1):]


def _outside_g1():
    """a point of order 11 on the curve, as blst_p1 bytes with Z != 1"""
    enc = [e for e in E.by_class(2) if e[0].startswith("order 11")][0][1]
    a, g = O.G1Affine(), O.G1()
    L = O.lib()
    assert L.og1_uncompress(C.byref(a), enc) and L.og1_affine_on_curve(C.byref(a))
    L.og1_from_affine(C.byref(g), C.byref(a))
    assert not L.og1_in_subgroup(C.byref(g))
    return _rescale(bytes(g), 3)


@pytest.mark.parametrize("n", [1, 2, 16])
def test_check_and_ok_each_agree_tuple_by_tuple(kzg, n):
    fs = kzg.FFTSettings(5)
    try:
        pool = _pool(n, _root(fs, n) if n > 1 else 1)
        other = _point_bytes(12345)
        gpu, host = _two_handles(kzg, fs, n)
        with gpu, host:
            for count in COUNTS:
                com, prf, xs, ys = _buffers(pool, count)
                last = count - 1
                cases = {"valid": (com, prf, ys),
                         "wrong y": (com, prf, _buffers(pool, count, (0, last))[3]),
                         "wrong proof": (com, _swap(prf, last, other), ys),
                         "wrong commitment": (_swap(com, count // 2, other), prf, ys),
                         "proof = identity": (com, _swap(prf, 0, ZERO_POINT), ys)}
                for what, (c, p, y) in cases.items():
                    got, want = gpu.check(c, p, xs, y, n, count), host.check(c, p, xs, y, n, count)
                    assert got == want, (what, n, count, [t for t in range(count) if got[t] != want[t]])
                    if what == "valid":
                        assert got == [True] * count
                    elif what == "wrong proof":
                        assert got[last] is False and all(got[:last])
                    # the ok_each of a failing batch is the per-tuple answer, through either handle
                    if what not in ("valid",):
                        vg, eg = gpu.check_batch(c, p, xs, y, n, count, each=True)
                        vh, eh = host.check_batch(c, p, xs, y, n, count, each=True)
                        assert (vg, eg) == (vh, eh), (what, n, count)
                        if not vg:
                            assert eg == got, (what, n, count)
    finally:
        fs.close()


@pytest.mark.parametrize("n", [1, 16])
def test_points_outside_g1_and_off_the_curve_reach_the_host_loop(kzg, n):
    fs = kzg.FFTSettings(5)
    try:
        pool = _pool(n, _root(fs, n) if n > 1 else 1)
        outside = _outside_g1()
        off = bytearray(pool["com"][1])
        off[0] ^= 1
        gpu, host = _two_handles(kzg, fs, n)
        with gpu, host:
            for count in (5, 70):
                com, prf, xs, ys = _buffers(pool, count)
                for what, c, p in (("proof outside G1", com, _swap(prf, 1, outside)),
                                   ("commitment outside G1", _swap(com, count - 1, outside), prf),
                                   ("both, and a wrong proof beside them", _swap(com, 0, outside), _swap(_swap(prf, 0, outside), 4, _point_bytes(7))),
                                   ("proof off the curve", com, _swap(prf, 4, bytes(off)))):
                    got, want = gpu.check(c, p, xs, ys, n, count), host.check(c, p, xs, ys, n, count)
                    assert got == want, (what, n, count, [t for t in range(count) if got[t] != want[t]])
                    assert any(got)  # the other tuples still pass
    finally:
        fs.close()


def test_error_codes_are_unchanged(kzg):
    L = kzg.lib()
    fs = kzg.FFTSettings(3)
    try:
        n = 4
        pool = _pool(n, _root(fs, n))
        com, prf, xs, ys = _buffers(pool, 3)
        zero_x = _fr_bulk([5, 0, 7])
        ok = (C.c_bool * 3)()
        gpu, host = _two_handles(kzg, fs, n)
        with gpu, host:
            for kz in (gpu, host):
                h = kz.handle
                assert L.kzgamd_kzg_check(h, ok, com, prf, xs, ys, n, 3) == 0 and list(ok) == [True] * 3
                assert L.kzgamd_kzg_check(h, ok, com, prf, zero_x, ys, n, 3) == 5      # x = 0 with n > 1
                assert L.kzgamd_kzg_check(h, ok, com, prf, xs, ys, 16, 3) == 4         # n > width
                assert L.kzgamd_kzg_check(h, ok, com, prf, xs, ys, 3, 3) == 3          # n no power of two
                assert L.kzgamd_kzg_check(h, ok, com, prf, xs, ys, 8, 3) == 6          # num_g2 = 5 <= 8
                assert L.kzgamd_kzg_check(h, None, com, prf, xs, ys, n, 3) == -1
                assert L.kzgamd_kzg_check(h, None, None, None, None, None, n, 0) == 0
    finally:
        fs.close()
