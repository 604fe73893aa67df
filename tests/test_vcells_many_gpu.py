"""kzgamd_verify_cell_kzg_proof_batch_many / _many_g1 on the GPU: many verify_cell_kzg_proof_batch inputs in one call
under one pairing (rust-kzg_amd/csrc/ckzg_vcells.hip).

The yardstick is the existing verify_cell_kzg_proof_batch, pinned on the reference's vectors by
tests/test_cells7594_gpu.py: per batch the new call must say what it says.  Cells and proofs come from four random blobs
through the product's own compute_cells_and_kzg_proofs, commitments from blob_to_kzg_commitment.  The combination
itself (outer weights, derived rho) is checked on the G1 pair against the library's own linear combination of the
nbatch = 1 pairs and against tests/vcells_many_model.py's byte layout."""
import ctypes as C
import gzip
import json
import os
import random
import threading

import pytest

import g1_encodings as E
import vcells_many_model as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
CELL = 2048
R = V.R
P = E.P
EMPTY = (b"", [], b"", b"")


def unhex(s):
    return bytes.fromhex(s[2:])


class World:
    pass


@pytest.fixture(scope="module")
def world(kzg):
    w = World()
    w.s = kzg.KZGSettings.from_file(os.path.join(GOLDEN, "trusted_setup.txt"))
    rnd = random.Random(7594)
    w.blobs = []
    for _ in range(4):
        b = bytearray(rnd.randbytes(131072))
        for i in range(0, 131072, 32):
            b[i] = 0
        w.blobs.append(bytes(b))
    w.cms = [kzg.blob_to_kzg_commitment(b, w.s) for b in w.blobs]
    w.cp = [kzg.compute_cells_and_kzg_proofs(b, w.s) for b in w.blobs]
    yield w
    w.s.close()


def tup(w, k, i):
    """(commitment, column, cell, proof) of blob k, column i"""
    return (w.cms[k], i, w.cp[k][0][CELL * i: CELL * (i + 1)], w.cp[k][1][48 * i: 48 * (i + 1)])


def batch(tuples):
    return (b"".join(t[0] for t in tuples), [t[1] for t in tuples], b"".join(t[2] for t in tuples), b"".join(t[3] for t in tuples))


def single(kzg, w, b):
    return kzg.verify_cell_kzg_proof_batch(b[0], b[1], b[2], b[3], w.s)


def agrees_with_single_calls(kzg, w, batches):
    want = [single(kzg, w, b) for b in batches]
    ok, each = kzg.verify_cell_kzg_proof_batch_many(batches, w.s)
    assert each == want and ok == all(want)
    return want


def fr_mont(kzg, v):
    return kzg.BlstFr.from_buffer_copy(((v << 256) % R).to_bytes(32, "little"))


def affine(p1):
    """a Jacobian BlstP1 (Montgomery limbs) -> (x, y) integers, None for the identity"""
    raw = bytes(p1)
    inv = pow(1 << 384, -1, P)
    x, y, z = (int.from_bytes(raw[48 * i: 48 * (i + 1)], "little") * inv % P for i in range(3))
    if z == 0:
        return None
    zi = pow(z, -1, P)
    return x * zi * zi % P, y * zi * zi * zi % P


def lincomb(kzg, points, scalars):
    """sum scalars[i] points[i] through the library's own variable-base MSM; identities are left out"""
    keep = [(affine(p), k) for p, k in zip(points, scalars)]
    keep = [(a, k) for a, k in keep if a is not None]
    if not keep:
        return None
    pts = (kzg.BlstP1Affine * len(keep))()
    sc = (kzg.BlstFr * len(keep))()
    for i, ((x, y), k) in enumerate(keep):
        C.memmove(C.byref(pts[i]), ((x << 384) % P).to_bytes(48, "little") + ((y << 384) % P).to_bytes(48, "little"), 96)
        sc[i] = fr_mont(kzg, k)
    return affine(kzg.multi_scalar_mult(pts, sc, len(keep)))


@pytest.fixture(scope="module")
def vec():
    with open(os.path.join(GOLDEN, "kzg_mainnet_7594.json")) as f:
        v = json.load(f)
    with gzip.open(os.path.join(GOLDEN, v["cells_file"]), "rb") as f:
        blob = f.read()
    v["_cells"] = [blob[i: i + CELL] for i in range(0, len(blob), CELL)]
    return v


def _expressible(vec):
    """the verify_cell_kzg_proof_batch cases that fit (pointer, num_cells): (name, batch, output)"""
    out = []
    for case in vec["verify_cell_kzg_proof_batch"]:
        refs = case["cells"]
        coms = [unhex(c) for c in case["commitments"]]
        prfs = [unhex(p) for p in case["proofs"]]
        n = len(case["cell_indices"])
        if any(isinstance(r, dict) for r in refs) or not (len(coms) == len(prfs) == len(refs) == n) or \
                any(len(c) != 48 for c in coms) or any(len(p) != 48 for p in prfs):
            assert case["output"] is None
            continue
        out.append((case["name"], (b"".join(coms), case["cell_indices"], b"".join(vec["_cells"][r] for r in refs), b"".join(prfs)),
                    case["output"]))
    return out


def test_reference_vectors_one_by_one_and_all_together(kzg, world, vec):
    cases = _expressible(vec)
    seen = {True: 0, False: 0, None: 0}
    for name, b, output in cases:
        if output is None:
            with pytest.raises(kzg.KzgAmdError):
                kzg.verify_cell_kzg_proof_batch_many([b], world.s)
        else:
            assert kzg.verify_cell_kzg_proof_batch_many([b], world.s) == (output, [output]), name
        seen[output] += 1
    assert seen[True] >= 12 and seen[False] >= 3 and seen[None] >= 1
    decided = [(b, o) for _, b, o in cases if o is not None]
    ok, each = kzg.verify_cell_kzg_proof_batch_many([b for b, _ in decided], world.s)
    assert each == [o for _, o in decided] and ok is False


def test_sidecar_shape_one_batch_per_column(kzg, world):
    w = world
    good = [[tup(w, k, c) for k in range(4)] for c in range(128)]
    assert kzg.verify_cell_kzg_proof_batch_many([batch(t) for t in good], w.s) == (True, [True] * 128)
    only37 = [c != 37 for c in range(128)]
    wrong = [list(t) for t in good]
    com, i, cell, _ = wrong[37][2]
    wrong[37][2] = (com, i, cell, tup(w, 2, 38)[3])  # a G1 point, the wrong proof
    assert kzg.verify_cell_kzg_proof_batch_many([batch(t) for t in wrong], w.s) == (False, only37)
    swapped = [list(t) for t in good]
    com, i, _, prf = swapped[37][1]
    swapped[37][1] = (com, i, tup(w, 3, 37)[2], prf)  # another blob's cell of that column
    assert kzg.verify_cell_kzg_proof_batch_many([batch(t) for t in swapped], w.s) == (False, only37)


def _challenge(kzg, b):
    """r_b of one batch through the existing challenge entry point: its own commitments, first appearances in order"""
    coms = [b[0][48 * i: 48 * (i + 1)] for i in range(len(b[1]))]
    uniq = list(dict.fromkeys(coms))
    return int.from_bytes(kzg.compute_verify_cell_kzg_proof_batch_challenge(b"".join(uniq), [uniq.index(c) for c in coms], b[1], b[2], b[3]), "big")


def test_pair_is_the_weighted_sum_of_the_single_batch_pairs(kzg, world):
    w = world
    rnd = random.Random(3)
    sizes = [3, 0, 1, 5, 0, 2]
    batches = [batch([tup(w, rnd.randrange(4), rnd.randrange(128)) for _ in range(m)]) for m in sizes]
    singles = [kzg.verify_cell_kzg_proof_batch_many_g1([b], w.s) for b in batches]
    assert affine(singles[1][0]) is None and affine(singles[1][1]) is None
    for rho in (1, rnd.randrange(R)):
        got = kzg.verify_cell_kzg_proof_batch_many_g1(batches, w.s, rho=fr_mont(kzg, rho))
        weights = [pow(rho, b, R) for b in range(len(sizes))]
        for side in (0, 1):
            assert affine(got[side]) == lincomb(kzg, [p[side] for p in singles], weights), (rho, side)
    # rho = NULL: derived from the batches' own challenges, in the documented layout
    rho = V.outer_challenge([_challenge(kzg, b) for b in batches])
    derived = kzg.verify_cell_kzg_proof_batch_many_g1(batches, w.s)
    given = kzg.verify_cell_kzg_proof_batch_many_g1(batches, w.s, rho=fr_mont(kzg, rho))
    assert [affine(p) for p in derived] == [affine(p) for p in given]
    assert affine(derived[0]) != affine(singles[0][0])
    # the pair of a valid call satisfies the pairing equation against [s^64]G2
    g2s64 = C.cast(C.c_void_p(w.s.c.g2_values_monomial), C.POINTER(kzg.BlstP2))[64]
    assert kzg.pairings_verify(derived[1], kzg.p2_generator(), derived[0], g2s64)
    assert not kzg.pairings_verify(derived[0], kzg.p2_generator(), derived[1], g2s64)
    zero = kzg.verify_cell_kzg_proof_batch_many_g1([], w.s)
    assert affine(zero[0]) is None and affine(zero[1]) is None


def test_outer_weights_catch_errors_that_cancel_unweighted(kzg, world):
    """two batches, each with cell 0 of the same column, proofs pi + D and pi' - D"""
    w = world
    d = E.mul(0x1234567, E.G)
    a, b = tup(w, 0, 0), tup(w, 1, 0)
    pa = E.compress(E.add(E.decode(a[3]), d))
    pb = E.compress(E.add(E.decode(b[3]), E.neg(d)))
    batches = [batch([(a[0], 0, a[2], pa)]), batch([(b[0], 0, b[2], pb)])]
    assert not single(kzg, w, batches[0]) and not single(kzg, w, batches[1])
    ok, each = kzg.verify_cell_kzg_proof_batch_many(batches, w.s, rho=fr_mont(kzg, 1))
    assert ok is True and each == [True, True]  # a rho known before the inputs: the errors cancel
    assert kzg.verify_cell_kzg_proof_batch_many(batches, w.s) == (False, [False, False])


def test_aggregation_slices_and_columns(kzg, world):
    w = world
    S = kzg.vcells_info()
    assert S >= 1
    # every cell of the call in one column
    for total in (1, S, S + 1, 2 * S + 1):
        tuples = [tup(w, k % 4, 5) for k in range(total)]
        assert agrees_with_single_calls(kzg, w, [batch(tuples)]) == [True]
        com, i, cell, _ = tuples[-1]
        tuples[-1] = (com, i, cell, tup(w, 0, 6)[3])
        assert agrees_with_single_calls(kzg, w, [batch(tuples)]) == [False]
        if total > 1:
            cut = total // 2
            assert agrees_with_single_calls(kzg, w, [batch(tuples[:cut]), batch(tuples[cut:])]) == [True, False]
    # columns with 0 / 1 / S + 1 cells, dealt round over three batches
    tuples = [tup(w, k % 4, c) for c in range(128) for k in range((0, 1, S + 1)[c % 3])]
    assert agrees_with_single_calls(kzg, w, [batch(tuples[j::3]) for j in range(3)]) == [True] * 3
    # a batch with more than 128 cells beside a small one
    big = [tup(w, k % 4, (7 * k) % 128) for k in range(200)]
    assert agrees_with_single_calls(kzg, w, [batch(big), batch(big[:3])]) == [True, True]
    big[150] = big[150][:3] + (big[151][3],)
    assert agrees_with_single_calls(kzg, w, [batch(big[:3]), batch(big)]) == [True, False]
    # the same commitment in every batch / a different one per batch
    for blob_of in (lambda b: 0, lambda b: b % 4):
        assert agrees_with_single_calls(kzg, w, [batch([tup(w, blob_of(b), (b + j) % 128) for j in range(3)]) for b in range(6)]) == [True] * 6


def test_16384_cells_in_one_call(kzg, world):
    w = world
    batches = [batch([tup(w, b % 4, c) for c in range(128)]) for b in range(128)]
    assert kzg.verify_cell_kzg_proof_batch_many(batches, w.s) == (True, [True] * 128)
    t = [tup(w, 0, c) for c in range(128)]
    t[127] = t[127][:3] + (t[126][3],)
    batches[100] = batch(t)
    assert agrees_with_single_calls(kzg, w, batches) == [b != 100 for b in range(128)]


def test_edges_and_rejections(kzg, world):
    w = world
    S = kzg.vcells_info()
    good = [batch([tup(w, 0, 1), tup(w, 1, 2)]), batch([tup(w, 2, 3)])]

    def still_fine():
        assert kzg.verify_cell_kzg_proof_batch_many(good, w.s) == (True, [True, True])

    def rejected(batches):
        with pytest.raises(kzg.KzgAmdError):
            kzg.verify_cell_kzg_proof_batch_many(batches, w.s)
        with pytest.raises(kzg.KzgAmdError):
            kzg.verify_cell_kzg_proof_batch_many_g1(batches, w.s)
        still_fine()  # nothing is left in flight

    assert kzg.verify_cell_kzg_proof_batch_many([], w.s) == (True, [])
    assert kzg.verify_cell_kzg_proof_batch_many([EMPTY] * 3, w.s) == (True, [True] * 3)
    assert kzg.verify_cell_kzg_proof_batch_many([EMPTY, good[1], EMPTY], w.s) == (True, [True] * 3)
    assert kzg.verify_cell_kzg_proof_batch_many(good, w.s, want_each=False) == (True, None)
    bad_proof = batch([tup(w, 2, 3)[:3] + (tup(w, 2, 4)[3],)])
    assert kzg.verify_cell_kzg_proof_batch_many([good[0], bad_proof], w.s, want_each=False) == (False, None)
    assert kzg.verify_cell_kzg_proof_batch_many([good[0], bad_proof], w.s) == (False, [True, False])
    # a cell element r - 1 is a scalar: accepted, and judged like the single call judges it
    com, i, cell, prf = tup(w, 0, 9)
    top = batch([(com, i, cell[:-32] + (R - 1).to_bytes(32, "big"), prf)])
    assert agrees_with_single_calls(kzg, w, [good[1], top]) == [True, False]
    # r is not: the last element of the last cell of the last slice of a column
    tuples = [tup(w, k % 4, 5) for k in range(2 * S + 1)]
    com, i, cell, prf = tuples[-1]
    tuples[-1] = (com, i, cell[:-32] + R.to_bytes(32, "big"), prf)
    rejected([good[0], batch(tuples)])
    rejected([good[0], batch([tup(w, 0, 1)[:1] + (128,) + tup(w, 0, 1)[2:]])])
    outside = dict(E.by_class(2))
    no_encoding = E.by_class(1)[0][1]
    com, i, cell, prf = tup(w, 3, 77)
    rejected([good[0], batch([(com, i, cell, outside["(0, 2)"])])])
    rejected([batch([(outside["order 11"], i, cell, prf)]), good[1]])
    rejected([good[0], good[1], batch([(com, i, cell, no_encoding)])])
    rejected([batch([(no_encoding, i, cell, prf)])])
    # NULL arguments
    L = kzg.lib()
    ok = C.c_bool(True)
    num = (C.c_uint64 * 1)(1)
    idx = (C.c_uint64 * 1)(i)
    sp = C.byref(w.s.c)
    assert L.kzgamd_verify_cell_kzg_proof_batch_many(None, None, com, idx, cell, prf, num, 1, None, sp) == kzg.C_KZG_BADARGS
    assert L.kzgamd_verify_cell_kzg_proof_batch_many(C.byref(ok), None, com, idx, cell, prf, None, 1, None, sp) == kzg.C_KZG_BADARGS
    assert L.kzgamd_verify_cell_kzg_proof_batch_many(C.byref(ok), None, com, idx, None, prf, num, 1, None, sp) == kzg.C_KZG_BADARGS
    assert L.kzgamd_verify_cell_kzg_proof_batch_many_g1(None, com, idx, cell, prf, num, 1, None, sp) == kzg.C_KZG_BADARGS
    assert ok.value is True  # nothing written
    assert L.kzgamd_verify_cell_kzg_proof_batch_many(C.byref(ok), None, com, idx, cell, prf, num, 1, None, sp) == kzg.C_KZG_OK
    assert ok.value is True
    still_fine()


def test_four_threads_on_one_settings_object(kzg, world):
    w = world
    good = [batch([tup(w, k, (11 * t + k) % 128) for k in range(4)]) for t in range(6)]
    bad = list(good)
    bad[4] = batch([tup(w, 0, 50)[:3] + (tup(w, 1, 50)[3],)])
    want_bad = [b != 4 for b in range(6)]
    assert kzg.verify_cell_kzg_proof_batch_many(good, w.s) == (True, [True] * 6)
    assert kzg.verify_cell_kzg_proof_batch_many(bad, w.s) == (False, want_bad)
    results = [None] * 4

    def work(t):
        try:
            results[t] = [kzg.verify_cell_kzg_proof_batch_many(good, w.s), kzg.verify_cell_kzg_proof_batch_many(bad, w.s),
                          kzg.verify_cell_kzg_proof_batch_many(good[t:], w.s)]
        except Exception as e:  # noqa: BLE001  (reported by the assertion below)
            results[t] = e

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for t in range(4):
        assert results[t] == [(True, [True] * 6), (False, want_bad), (True, [True] * (6 - t))], (t, results[t])
