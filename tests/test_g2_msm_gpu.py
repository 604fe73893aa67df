"""kzgamd_g2_msm on the handle of kzgamd_g2_msm_new (g2msm.hip: a table 2^(8k) P_i, the signed base-256 digits of a call
sorted into 128 buckets per batch item, the buckets cut into segments that a lane each adds up, level by level, and the
bucket sums weighted by their indices) through the C ABI, on both library flavours.

Anchors: up to 257 points the host loop of kzgamd_p2_mult / kzgamd_p2_add (host_pairing.h), compared through
kzgamd_p2_compress; above, kzgamd_g2_lincomb on the same inputs.  Every output of every call is checked for its form (Z
== one, or all-zero for the identity), and every call is made twice and must return the same bytes.  Every reference
sum is computed once per process and shared by the two flavours.

The counts are the smallest at which each stage can go wrong: a count workgroup not full, full, one lane into the second
(63, 64, 65), and 257 = 5 of them; with g2msm_segment=4 and every entry in one bucket, counts that fill, end and begin a
segment at the first, second and third level (3, 4, 5, 16, 17, 64, 65); with g2msm_pass_entries=32 and 64 one and two
points per pass."""
import ctypes as C
import random
import threading

import pytest

import setup_model as S
from test_g2_lincomb_gpu import INF2, host_sum, neg_p2, p2_array, pool
from test_group_mul_gpu import fr_bulk, p2_from_affine, twist_bases

pytestmark = pytest.mark.gpu
R = S.R
CASES = S.scalar_cases()
ONES32 = int.from_bytes(b"\x01" * 32, "little")  # the digit 1 in every window
MALFORMED = ("g2msm_segment=1", "g2msm_segment=24", "g2msm_segment=", "g2msm_pass_entries=16", "g2msm_pass_entries=48", "spl=1")


def mixed(kzg, n, seed):
    rnd = random.Random(seed)
    pts = pool(kzg)
    return [pts[rnd.randrange(len(pts))] for _ in range(n)], [rnd.randrange(R) for _ in range(n)]


def check_form(kzg, out, nbatch):
    """every output is all-zero, or has Z == one (the generator's Z) — and canonical coordinates, which p2_compress reads"""
    one = pool(kzg)[0][192:288]
    raw = bytes(out)
    for b in range(nbatch):
        p = raw[288 * b:288 * b + 288]
        assert p == bytes(288) or p[192:288] == one, b
    return [raw[288 * b:288 * b + 288] for b in range(nbatch)]


def call(kzg, h, vals, n, nbatch=1):
    """the outputs of one call as bytes, made twice"""
    sc = fr_bulk(kzg, vals)
    got = check_form(kzg, h.g2_msm(sc, n, nbatch), nbatch)
    assert check_form(kzg, h.g2_msm(sc, n, nbatch), nbatch) == got, "a repeated call returns the same bytes"
    return got


def compressed(kzg, raw288):
    p = kzg.BlstP2()
    C.memmove(C.byref(p), raw288, 288)
    return kzg.p2_compress(p)


def check(kzg, key, raw, vals, h=None, config=None, expect_identity=None):
    """one linear combination over raw (the first len(raw) points of h, or a handle of its own) against the host loop"""
    n = len(raw)
    own = h is None
    if own:
        h = kzg.G2Msm(p2_array(kzg, raw), n, config)
    try:
        got = call(kzg, h, vals, n)[0]
    finally:
        if own:
            h.close()
    want = host_sum(kzg, ("g2msm", key), raw, vals)
    assert compressed(kzg, got) == want, key
    if want == INF2:
        assert got == bytes(288), (key, "the identity is all-zero")
    if expect_identity is not None:
        assert (want == INF2) == expect_identity, key
    return got


def test_counts_and_the_prefix_rule(kzg):
    raw, vals = mixed(kzg, 257, 1257)
    h = kzg.G2Msm(p2_array(kzg, raw), 257)
    try:
        for n in (0, 1, 2, 3, 63, 64, 65, 257):
            check(kzg, ("count", n), raw[:n], vals[:n], h=h, expect_identity=(n == 0))
        out = (kzg.BlstP2 * 1)()
        assert kzg.lib().kzgamd_g2_msm(h.handle, out, fr_bulk(kzg, vals + [1]), 258, 1) == 1
    finally:
        h.close()


def test_every_scalar_case_in_one_call(kzg):
    assert len(CASES) == 872
    pts = pool(kzg)
    check(kzg, "scalar cases", [pts[i % len(pts)] for i in range(len(CASES))], CASES)


def test_digit_edges(kzg):
    raw, _ = mixed(kzg, 70, 5)
    h = kzg.G2Msm(p2_array(kzg, raw), 70)
    try:
        vectors = [("128: bucket 128", 128), ("129: digit -127 and a carry", 129), ("255", 255), ("256", 256), ("r - 1", R - 1),
                   ("zero", 0), ("one", 1), ("all equal", CASES[-1])]
        got = call(kzg, h, [v for _, v in vectors for _ in range(70)], 70, len(vectors))
        for (tag, v), g in zip(vectors, got):
            want = host_sum(kzg, ("g2msm", "digit edge", tag), raw, [v] * 70)
            assert compressed(kzg, g) == want, tag
            assert (g == bytes(288)) == (want == INF2) == (v == 0), tag
    finally:
        h.close()


def test_segment_and_level_edges(kzg):
    raw, _ = mixed(kzg, 65, 11)
    cfg = kzg.make_config(tuning="g2msm_segment=4")
    h = kzg.G2Msm(p2_array(kzg, raw), 65, cfg)
    try:
        assert h.info()["segment"] == 4
        for n in (3, 4, 5, 16, 17, 64, 65):  # n entries in bucket 1
            check(kzg, ("all one", n), raw[:n], [1] * n, h=h)
        check(kzg, ("32 bytes of 1", 17), raw[:17], [ONES32] * 17, h=h)  # 544 entries in bucket 1: five levels
    finally:
        h.close()
    raw, _ = mixed(kzg, 257, 12)
    h = kzg.G2Msm(p2_array(kzg, raw), 257)
    try:
        check(kzg, ("all one", 257), raw, [1] * 257, h=h)
        check(kzg, ("32 bytes of 1", 257), raw, [ONES32] * 257, h=h)  # 8224 entries in bucket 1
    finally:
        h.close()


@pytest.mark.parametrize("cap", [32, 64])
def test_passes(kzg, cap):
    raw, vals = mixed(kzg, 5, 21)
    h = kzg.G2Msm(p2_array(kzg, raw), 5, kzg.make_config(tuning="g2msm_pass_entries=%d" % cap))
    try:
        assert h.info()["pass_entries"] == cap
        for n in (1, 2, 3, 5):
            check(kzg, ("passes", n), raw[:n], vals[:n], h=h)
        # a batch under the cap: one item per pass (32), or two (64, one point each)
        got = call(kzg, h, vals[:1] + vals[1:2] + vals[2:3], 1, 3)
        for b in range(3):
            assert compressed(kzg, got[b]) == host_sum(kzg, ("g2msm", "passes, batch", b), raw[:1], vals[b:b + 1])
    finally:
        h.close()


def test_equal_points_every_addition_a_doubling(kzg):
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
    check(kzg, "64 P then 64 -P", raw[:64] + [neg_p2(r) for r in raw[:64]], vals[:64] * 2, expect_identity=True)


def test_points_at_infinity(kzg):
    raw, vals = mixed(kzg, 130, 6)
    junk = random.Random(8).randbytes(192) + bytes(96)  # Z == 0 is the identity whatever X and Y hold
    some = [bytes(288) if i % 5 == 1 else junk if i % 7 == 3 else r for i, r in enumerate(raw)]
    check(kzg, "some at infinity", some, vals, expect_identity=False)
    check(kzg, "all at infinity", [bytes(288), junk] * 40, vals[:80], expect_identity=True)


@pytest.mark.parametrize("which", ["order13", "full"])
def test_points_outside_the_subgroup_still_sum_by_the_group_law(kzg, which):
    base = bytes(p2_from_affine(kzg, twist_bases()[which]))
    pts = pool(kzg)
    vals = list(range(0, 30)) + [13 * 256 ** 7, R - 1] + CASES[6::40]
    raw = [base if i % 2 == 0 else pts[i % len(pts)] for i in range(len(vals))]
    check(kzg, ("outside", which), raw, vals)
    check(kzg, ("outside alone", which), [base] * 27, list(range(27)), expect_identity=(which == "order13"))  # sum 0..26 = 27 * 13


def test_batches(kzg):
    raw, vals = mixed(kzg, 70, 31)
    h = kzg.G2Msm(p2_array(kzg, raw), 70)
    try:
        vectors = [vals, [0] * 70, [1] * 70]
        got = call(kzg, h, vectors[0] + vectors[1] + vectors[2], 70, 3)
        for b in range(3):
            assert call(kzg, h, vectors[b], 70) == [got[b]], b
            assert compressed(kzg, got[b]) == host_sum(kzg, ("g2msm", "batch", b), raw, vectors[b]), b
        assert got[1] == bytes(288)
        # nbatch == 0: nothing is written, no pointer is looked at
        out = (kzg.BlstP2 * 2)()
        C.memset(out, 0xa5, C.sizeof(out))
        assert kzg.lib().kzgamd_g2_msm(h.handle, out, fr_bulk(kzg, vals), 70, 0) == 0 and bytes(out) == b"\xa5" * 576
        assert kzg.lib().kzgamd_g2_msm(h.handle, None, None, 70, 0) == 0
        # n == 0: identities
        assert kzg.lib().kzgamd_g2_msm(h.handle, out, None, 0, 2) == 0 and bytes(out) == bytes(576)
    finally:
        h.close()


def test_against_the_walk_at_4097_points(kzg):
    raw, vals = mixed(kzg, 4097, 4097)
    pts, sc = p2_array(kzg, raw), fr_bulk(kzg, vals)
    h = kzg.G2Msm(pts, 4097)
    try:
        info = h.info()
        assert info["npoints"] == 4097 and info["window_bits"] == 8 and info["table_bytes"] == 4097 * 32 * 240
        got = check_form(kzg, h.g2_msm(sc, 4097, 1), 1)
        assert check_form(kzg, h.g2_msm(sc, 4097, 1), 1) == got
    finally:
        h.close()
    assert compressed(kzg, got[0]) == kzg.p2_compress(kzg.g2_lincomb(pts, sc, 4097)) != INF2


def test_null_pointers_tuning_keys_budget_and_info(kzg):
    L = kzg.lib()
    raw, vals = mixed(kzg, 3, 2)
    pts, sc, out = p2_array(kzg, raw), fr_bulk(kzg, vals), (kzg.BlstP2 * 1)()
    err = C.c_int(99)
    assert L.kzgamd_g2_msm_new(None, 3, None, C.byref(err)) is None and err.value == -1
    assert L.kzgamd_g2_msm_new(None, 3, None, None) is None  # err may be NULL
    for bad in MALFORMED:
        cfg = kzg.make_config(tuning=bad)
        err.value = 99
        assert L.kzgamd_g2_msm_new(pts, 3, C.byref(cfg), C.byref(err)) is None and err.value == -2, bad
    keys = kzg.tuning_keys()
    assert "g2msm_segment" not in keys and "g2msm_pass_entries" not in keys
    h = kzg.G2Msm(pts, 3, kzg.make_config(tuning="g2msm_segment=8;g2msm_pass_entries=96"))
    try:
        assert h.info() == {"npoints": 3, "window_bits": 8, "segment": 8, "pass_entries": 96, "table_bytes": 3 * 32 * 240}
        assert L.kzgamd_g2_msm(h.handle, None, sc, 3, 1) == -1
        assert L.kzgamd_g2_msm(h.handle, out, None, 3, 1) == -1
        assert L.kzgamd_g2_msm(None, out, sc, 3, 1) == -1
        assert L.kzgamd_g2_msm_info(None, None, None, None, None, None) == -1
        assert L.kzgamd_g2_msm_info(h.handle, None, None, None, None, None) == 0
        check(kzg, ("keys", 3), raw, vals, h=h)
    finally:
        h.close()
    L.kzgamd_g2_msm_free(None)
    # the budget: one byte below the table fails with 2, the table's own size passes
    cfg = kzg.make_config()
    cfg.table_budget_bytes = 3 * 32 * 240 - 1
    err.value = 99
    assert L.kzgamd_g2_msm_new(pts, 3, C.byref(cfg), C.byref(err)) is None and err.value == 2
    cfg.table_budget_bytes = 3 * 32 * 240
    h = kzg.G2Msm(pts, 3, cfg)
    h.close()
    # no points: every sum is the identity
    h = kzg.G2Msm(None, 0)
    try:
        assert call(kzg, h, [], 0, 2) == [bytes(288)] * 2
        assert L.kzgamd_g2_msm(h.handle, out, sc, 1, 1) == 1
    finally:
        h.close()


def test_create_and_free_returns_hbm(kzg):
    import torch

    raw, vals = mixed(kzg, 4096, 77)
    pts, sc = p2_array(kzg, raw), fr_bulk(kzg, vals)

    def cycle():
        h = kzg.G2Msm(pts, 4096)  # a table of 31 MB, and the workspace of a call
        try:
            return bytes(h.g2_msm(sc, 4096, 1))
        finally:
            h.close()

    first = cycle()  # the runtime's own one-off allocations happen here
    torch.cuda.synchronize()
    base_free, _ = torch.cuda.mem_get_info(0)
    for k in range(3):
        assert cycle() == first
        torch.cuda.synchronize()
        free, _ = torch.cuda.mem_get_info(0)
        assert base_free - free <= 8 << 20, (k, base_free - free)  # the allocator's granularity, as test_lifecycle_gpu.py has it


def test_four_threads_on_one_handle_get_the_single_thread_bytes(kzg):
    raw, vals = mixed(kzg, 130, 41)
    h = kzg.G2Msm(p2_array(kzg, raw), 130)
    try:
        inputs = [(vals[:n], n) for n in (130, 65, 64)]
        want = [call(kzg, h, v, n) for v, n in inputs]
        errs = []

        def work(t):
            try:
                for k in range(3):
                    v, n = inputs[(t + k) % 3]
                    assert check_form(kzg, h.g2_msm(fr_bulk(kzg, v), n, 1), 1) == want[(t + k) % 3]
            except Exception as e:  # noqa: BLE001
                errs.append((t, repr(e)))

        ts = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for th in ts:
            th.start()
        for th in ts:
            th.join()
        assert errs == []
    finally:
        h.close()
