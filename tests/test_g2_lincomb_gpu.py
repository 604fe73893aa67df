"""kzgamd_g2_lincomb (setupcheck.hip: a lane per point walks its scalar, a workgroup's 64 terms are summed through LDS,
the workgroups' sums by further launches) through the C ABI, on both library flavours.  The anchor is a host loop of
kzgamd_p2_mult / kzgamd_p2_add (host_pairing.h), compared through kzgamd_p2_compress; an identity must come out all-zero.

The counts are the smallest at which each stage can go wrong: one workgroup not full, full, one lane into the second
(63, 64, 65), a third workgroup begun (129), and 257 = 5 workgroups, whose sums take one launch of the sum kernel with
59 idle lanes; with lincomb_slice=64 the same counts end a slice, begin a second with one point, and sum three slice
sums.  Every reference sum is computed once per process and shared by the two flavours."""
import ctypes as C
import random

import pytest

import g1_encodings as E
import setup_model as S
from test_group_mul_gpu import fr_bulk, p2_from_affine, twist_bases

pytestmark = pytest.mark.gpu
R = S.R
CASES = S.scalar_cases()
INF2 = bytes([0xc0]) + bytes(95)
_ref = {}


def pool(kzg):
    """16 points of G2 as bytes: the generator (Z = 1) and multiples from the host's double-and-add (Z != 1)"""
    if "pool" not in _ref:
        g = kzg.p2_generator()
        pts = [bytes(g)] + [bytes(kzg.p2_mult(g, fr_bulk(kzg, [k])[0])) for k in range(2, 17)]
        assert all(p[192:288] != pts[0][192:288] for p in pts[1:])  # another Z than one
        _ref["pool"] = pts
    return _ref["pool"]


def p2_array(kzg, raw):
    arr = (kzg.BlstP2 * max(len(raw), 1))()
    if raw:
        C.memmove(arr, b"".join(raw), 288 * len(raw))
    return arr


def neg_p2(raw):
    """-P: the two components of Y negated mod p (Montgomery residues negate like plain ones)"""
    y = [(E.P - int.from_bytes(raw[96 + 48 * k:144 + 48 * k], "little")) % E.P for k in range(2)]
    return raw[:96] + b"".join(v.to_bytes(48, "little") for v in y) + raw[192:]


def host_sum(kzg, key, raw, vals):
    """compressed sum_i vals[i] * raw[i] by the host loop, once per key"""
    if key not in _ref:
        sc = fr_bulk(kzg, vals)
        acc = kzg.BlstP2()
        for i, r in enumerate(raw):
            p = kzg.BlstP2()
            C.memmove(C.byref(p), r, 288)
            acc = kzg.p2_add(acc, kzg.p2_mult(p, sc[i]))
        _ref[key] = kzg.p2_compress(acc)
    return _ref[key]


def check(kzg, key, raw, vals, config=None, expect_identity=None):
    n = len(raw)
    got = kzg.g2_lincomb(p2_array(kzg, raw), fr_bulk(kzg, vals), n, config=config)
    want = host_sum(kzg, key, raw, vals)
    assert kzg.p2_compress(got) == want, key
    if want == INF2:
        assert bytes(got) == bytes(288), (key, "the identity is all-zero")
    if expect_identity is not None:
        assert (want == INF2) == expect_identity, key


def mixed(kzg, n, seed):
    rnd = random.Random(seed)
    pts = pool(kzg)
    return [pts[rnd.randrange(len(pts))] for _ in range(n)], [rnd.randrange(R) for _ in range(n)]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 257])
def test_counts_with_random_scalars(kzg, n):
    raw, vals = mixed(kzg, n, 1000 + n)
    check(kzg, ("count", n), raw, vals, expect_identity=(n == 0))


@pytest.mark.parametrize("n", [64, 65, 129])
def test_slice_edges_and_the_sum_of_slice_sums(kzg, n):
    raw, vals = mixed(kzg, n, 1000 + n)  # the inputs (and the reference) of the unsliced run
    check(kzg, ("count", n), raw, vals, config=kzg.make_config(tuning="lincomb_slice=64"))


def test_special_scalars(kzg):
    raw, _ = mixed(kzg, 70, 5)
    check(kzg, "all zero", raw, [0] * 70, expect_identity=True)
    check(kzg, "all one", raw, [1] * 70, expect_identity=False)
    check(kzg, "all r - 1", raw, [R - 1] * 70, expect_identity=False)
    check(kzg, "all equal", raw, [CASES[-1]] * 70, expect_identity=False)
    check(kzg, "0, 1, r - 1 in turn", raw, [(0, 1, R - 1)[i % 3] for i in range(70)])


def test_every_scalar_case(kzg):
    assert len(CASES) == 872
    pts = pool(kzg)
    check(kzg, "scalar cases", [pts[i % len(pts)] for i in range(len(CASES))], CASES)


def test_points_at_infinity(kzg):
    raw, vals = mixed(kzg, 130, 6)
    junk = random.Random(8).randbytes(192) + bytes(96)  # Z == 0 is the identity whatever X and Y hold
    some = [bytes(288) if i % 5 == 1 else junk if i % 7 == 3 else r for i, r in enumerate(raw)]
    check(kzg, "some at infinity", some, vals, expect_identity=False)
    check(kzg, "all at infinity", [bytes(288), junk] * 40, vals[:80], expect_identity=True)


def test_equal_points_every_tree_addition_a_doubling(kzg):
    p = pool(kzg)[3]
    for n in (64, 128, 257):
        check(kzg, ("equal", n), [p] * n, [5] * n, expect_identity=False)


def test_opposite_points_sum_to_the_all_zero_identity(kzg):
    raw, vals = mixed(kzg, 65, 9)
    pairs, sc = [], []
    for r, v in zip(raw, vals):
        pairs += [r, neg_p2(r)]
        sc += [v, v]
    check(kzg, "P, -P", pairs, sc, expect_identity=True)
    # the two halves of a workgroup cancel at the last level of its tree
    check(kzg, "64 P then 64 -P", raw[:64] + [neg_p2(r) for r in raw[:64]], vals[:64] * 2, expect_identity=True)


@pytest.mark.parametrize("which", ["order13", "full"])
def test_points_outside_the_subgroup_still_sum_by_the_group_law(kzg, which):
    base = bytes(p2_from_affine(kzg, twist_bases()[which]))
    pts = pool(kzg)
    vals = list(range(0, 30)) + [13 * 256 ** 7, R - 1] + CASES[6::40]
    raw = [base if i % 2 == 0 else pts[i % len(pts)] for i in range(len(vals))]
    check(kzg, ("outside", which), raw, vals)
    check(kzg, ("outside alone", which), [base] * 27, list(range(27)), expect_identity=(which == "order13"))  # sum 0..26 = 27 * 13


def test_null_pointers_and_the_one_tuning_key(kzg):
    L = kzg.lib()
    raw, vals = mixed(kzg, 3, 2)
    pts, sc, out = p2_array(kzg, raw), fr_bulk(kzg, vals), kzg.BlstP2()
    assert L.kzgamd_g2_lincomb(None, pts, sc, 3, None) == -1
    assert L.kzgamd_g2_lincomb(C.byref(out), None, sc, 3, None) == -1
    assert L.kzgamd_g2_lincomb(C.byref(out), pts, None, 3, None) == -1
    C.memset(C.byref(out), 0x5a, 288)
    assert L.kzgamd_g2_lincomb(C.byref(out), None, None, 0, None) == 0 and bytes(out) == bytes(288)
    for bad in ("lincomb_slice=63", "lincomb_slice=32", "lincomb_slice=96", "mul_slice=64", "no_such_key=1", "spl=1"):
        cfg = kzg.make_config(tuning=bad)
        assert L.kzgamd_g2_lincomb(C.byref(out), pts, sc, 3, C.byref(cfg)) == -2, bad
    assert "lincomb_slice" not in kzg.tuning_keys()
    assert kzg.g2_lincomb_info() >= 64
