"""The bucket-edge cases of the variable-base MSM engine, checked without a GPU (tests/bucket_plan.py):
the recoding restated in Python is the signed-digit recoding; the constants the cases are derived from are the ones in
msm.hip; every named case really contains the edge it is named after (exact counts, piece counts, residues of the bucket
starts modulo the chunk, segments of k_heavy's first pass, heavy buckets per launch); and the group-sum reference the GPU
module compares against equals the oracle's Pippenger on scaled-down copies of every case (HEAVY = HSEG = 4, chunk 2)."""
import ctypes as C
import os
import random
import re

import pytest

import bucket_plan as bp
import oracle_ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, S = bp.HEAVY, bp.HSEG


# ---------------------------------------------------------------- the source's constants
def _source():
    with open(os.path.join(ROOT, "rust-kzg_amd", "csrc", "msm.hip")) as f:
        return f.read()


def test_constants_match_the_source():
    """whoever changes HEAVY, HSEG, the grid of k_heavy's first pass, the set limit of the top-of-tree forms or the choice
    of the chunk has to re-derive the cases"""
    src = _source()
    assert int(re.search(r"constexpr u32 HEAVY = (\d+);", src).group(1)) == bp.HEAVY
    assert int(re.search(r"constexpr u32 HSEG = (\d+);", src).group(1)) == bp.HSEG
    assert "const bool hv = cntb > HEAVY;" in src and "const bool hv = v > HEAVY;" in src  # k_bin_sort, k_scan
    m = re.search(r"int lgc = npoints >= \(\(size_t\)1 << (\d+)\) \? (\d+) : npoints >= \(\(size_t\)1 << (\d+)\) \? (\d+) : "
                  r"npoints >= \(\(size_t\)1 << (\d+)\) \? (\d+)\s*: npoints >= \(\(size_t\)1 << (\d+)\) \? (\d+) : (\d+);", src)
    assert m, "the host's choice of lgc has changed shape"
    g = [int(x) for x in m.groups()]
    assert tuple((1 << g[i], g[i + 1]) for i in range(0, 8, 2)) + ((0, g[8]),) == bp.LGC_BY_SIZE
    assert "int lgc_lo = lgc > 6 ? lgc - 2 : (lgc > 4 ? 4 : lgc);" in src
    assert "const ChunkSel csel{lgc_lo, lgc, (u32)(%d / nsets)};" % bp.LANE_TARGET in src
    assert re.search(r"k_heavy, dim3\(%d, 64\), dim3\(64\)" % bp.K_HEAVY_GRID_X, src)
    assert "const bool use_top = nsets <= %d;" % bp.USE_TOP_MAX_SETS in src
    assert re.search(r"while \(l > cs\.lo && \(total >> l\) < cs\.target\) --l;", src)
    assert [bp.default_lgc(n) for n in (1, 1 << 15, 1 << 18, 1 << 19, 1 << 20, 1 << 22)] == \
           [(4, 4), (4, 4), (5, 4), (6, 4), (7, 5), (8, 6)]


# ---------------------------------------------------------------- the recoding
def _edge_scalars(c):
    half, nw = 1 << (c - 1), bp.nwin_for(c)
    top = c * (nw - 1)
    out = [0, 1, bp.R - 1, half, half + 1, (half << top) % bp.R, ((half + 1) << top) % bp.R]
    out += [bp.structured_scalar(d, c, J) for d in (1, 2, half - 1, half) for J in (1, 3, 11) if c * J <= 250]
    return out


@pytest.mark.parametrize("c", [2, 5, 6, 11, 13, 16])
def test_recoding_identities(c):
    """sum digit_w 2^(c w) == s and every digit in (-2^(c-1), 2^(c-1)]: with the tie rule (d == half stays positive, which
    the range states) these determine the recoding"""
    rnd = random.Random(c)
    half, nw = 1 << (c - 1), bp.nwin_for(c)
    scalars = _edge_scalars(c) + [rnd.randrange(bp.R) for _ in range(300)] + [rnd.getrandbits(b) for b in (7, 64, 128, 129)]
    for s in scalars:
        digs = bp.signed_digits(s, c, nw)
        assert len(digs) == nw
        assert sum(d << (c * w) for w, d in enumerate(digs)) == s, (c, s)
        assert all(-half < d <= half for d in digs), (c, s)
    assert bp.signed_digits(half, c, nw)[:2] == [half, 0]
    assert bp.signed_digits(half + 1, c, nw)[:2] == [-(half - 1), 1]
    for d in (1, half - 1, half):
        for J in (1, 3):
            assert bp.signed_digits(bp.structured_scalar(d, c, J), c, nw) == [d] * J + [0] * (nw - J)


# ---------------------------------------------------------------- each case reaches its edge
def _plan(case, lgc=None, msm=0, **kw):
    lgc = lgc if lgc is not None else (case.lgc if case.lgc is not None else bp.default_lgc(case.n)[0])
    sc = case.scalars[msm * case.n:(msm + 1) * case.n]
    return bp.plan(sc, bp.live_mask(case), case.c, bp.nwin_for(case.c), lgc, **kw)


def _by_digit(st):
    return {b.bucket + 1: b for b in st["buckets"]}


def _same_first_sets(sets, J):
    """the first J sets are identical, the others empty"""
    assert all(s["buckets"] == sets[0]["buckets"] for s in sets[:J])
    assert all(s["total"] == 0 and not s["buckets"] for s in sets[J:])
    assert len(sets) > J  # empty upper sets are part of the case


def test_case_threshold():
    case = bp.case_threshold()
    assert case.n < 1 << 15  # one-level sort
    sets = _plan(case)
    _same_first_sets(sets, 3)
    b = _by_digit(sets[0])
    half = 1 << (case.c - 1)
    assert [(d, b[d].count, b[d].heavy) for d in sorted(b)] == [(1, H - 1, False), (7, H, False), (300, H + 1, True), (half, H, False)]
    assert b[half].bucket == (1 << (case.c - 1)) - 1  # the last bucket of the set
    # the last group has H + 1 bases of which one is infinity: without the live mask it would be flagged
    dead = bp.plan(case.scalars, [True] * case.n, case.c, bp.nwin_for(case.c), 4)
    assert _by_digit(dead[0])[half].count == H + 1


def test_case_alignment():
    case = bp.case_alignment()
    Cn = 1 << bp.default_lgc(case.n)[0]
    assert Cn == 16 and case.n < 1 << 15
    sets = _plan(case)
    _same_first_sets(sets, 3)
    b = _by_digit(sets[0])
    for d, a in ((2, 1), (5, Cn - 1)):
        assert b[d].heavy and b[d].beg % Cn == a  # begins a entries after a chunk start
        assert b[d].end % Cn == 1  # its last piece holds one entry
        assert b[d].pieces == (H + Cn) // Cn + 1 == 34
    for d in (3, 6):
        assert b[d].heavy and b[d].end % Cn == 0  # ends exactly at a chunk end
    last = b[1 << (case.c - 1)]
    assert last.heavy and last.beg % Cn == 0 and last.count == H + 1 and last.bucket == (1 << (case.c - 1)) - 1
    assert last.pieces == 33 and last.end % Cn == 1
    assert all(x.segments == 1 for x in sets[0]["buckets"])


def _check_segment_shapes(b, Cn):
    assert b[1].bucket == 0 and b[1].heavy and (b[1].count, b[1].beg % Cn, b[1].pieces, b[1].segments) == (S * Cn, 0, S, 1)
    assert b[2].heavy and (b[2].count, b[2].beg % Cn, b[2].pieces, b[2].segments) == (S * Cn + 1, 0, S + 1, 2)
    assert (b[2].pieces - 1) % S == 0  # the second segment has one element
    assert b[4].heavy and (b[4].count, b[4].beg % Cn, b[4].pieces, b[4].segments) == (2 * S * Cn + 1, 0, 2 * S + 1, 3)
    assert b[6].count == 1 and b[6].beg % Cn == 0
    assert b[7].heavy and (b[7].count, b[7].beg % Cn, b[7].pieces, b[7].segments) == (S * Cn, 1, S + 1, 2)


def test_case_segments():
    case = bp.case_segments()
    assert case.lgc == 2 and case.n < 1 << 15 and 20000 < case.n < 22000
    sets = _plan(case)
    _same_first_sets(sets, 3)
    _check_segment_shapes(_by_digit(sets[0]), 4)


@pytest.mark.parametrize("one_bin", [False, True])
def test_case_segments_default_chunk(one_bin):
    case = bp.case_segments_default_chunk(one_bin=one_bin)
    assert case.n == 1 << 15 and bp.default_lgc(case.n) == (4, 4)  # the two-level sort is taken from 2^15 entries on
    sets = _plan(case)
    _same_first_sets(sets, 3)
    b = _by_digit(sets[0])
    assert b[1].heavy and (b[1].count, b[1].pieces, b[1].segments) == (16 * S + 1, S + 1, 2)
    assert all(b[d].count == H + 1 and b[d].heavy and b[d].segments == 1 for d in range(2, 22))
    assert len(sets[0]["buckets"]) == 22 and len(bp.heavy_buckets(sets)) == 3 * 22
    last = sets[0]["buckets"][-1]
    half = 1 << (case.c - 1)
    if one_bin:
        assert all(x.bucket >> 7 == 0 for x in sets[0]["buckets"])  # one coarse bin of 2^7 fine buckets
    else:
        assert last.bucket == half - 1 and last.heavy
    assert sets[0]["total"] < case.n  # zero scalars fill up


def test_case_many_heavy():
    case = bp.case_many_heavy()
    sets = _plan(case)
    _same_first_sets(sets, 11)
    hv = bp.heavy_buckets(sets)
    assert len(hv) == 24 * 11 > bp.K_HEAVY_GRID_X
    assert all(x.count == H + 1 for x in hv)


@pytest.mark.parametrize("rot", range(4))
def test_case_exceptional(rot):
    case = bp.case_exceptional(rot)
    seg = bp.case_segments()
    big = lambda cs: [(g.digit, g.count) for g in cs.groups[0] if g.digit in (1, 2, 4, 7)]
    assert big(case) == big(seg)  # (the small groups that restore the alignment follow the live counts)
    sets = _plan(case)
    _same_first_sets(sets, 3)
    b = _by_digit(sets[0])
    mult = {}
    for k, d in enumerate((1, 2, 4, 7)):
        g = next(g for g in case.groups[0] if g.digit == d)
        kinds = case.kinds[g.start:g.start + g.count]
        variant = (rot + k) % 4
        mult[variant] = bp.exceptional_multiple(kinds)
        live = sum(x != bp.INF for x in kinds)
        assert b[d].heavy and b[d].count == live and b[d].pieces >= live // 4 > 64  # more pieces than a wave has lanes
        if variant == 0:
            assert live == g.count == mult[0]
        if variant == 3:
            assert sum(x == bp.INF for x in kinds) >= g.count // 5
        else:
            assert g.count - live <= 1
        if variant:
            assert any(x[0] == bp.NEGATED for x in kinds if x != bp.INF)
    assert (mult[1], mult[2], mult[3]) == (0, 3, 3)
    assert max(x.segments for x in sets[0]["buckets"]) >= 2  # and the tree of pass 2 sees such sums too


def test_case_batch3():
    case = bp.case_batch3()
    nw = bp.nwin_for(case.c)
    assert case.nbatch == 3 and 3 * nw <= bp.USE_TOP_MAX_SETS and case.n < 1 << 15
    _check_segment_shapes(_by_digit(_plan(case, msm=0)[0]), 4)
    assert all(s["total"] == 0 for s in _plan(case, msm=1))
    sets = _plan(case, msm=2)
    _same_first_sets(sets, 3)
    (only,) = sets[0]["buckets"]
    assert only.count == case.n > S * 4 and only.segments == -(-case.n // (4 * S)) == 6


def test_case_batch70():
    case = bp.case_batch70()
    assert case.nbatch * bp.nwin_for(case.c) > bp.USE_TOP_MAX_SETS and 4100 < case.n < 4300
    digits = set()
    for m in range(case.nbatch):
        sets = _plan(case, msm=m)
        _same_first_sets(sets, 3)
        (big,) = [x for x in sets[0]["buckets"] if x.heavy]
        assert big.count == 4 * S + 1 and big.segments == 2 and big.pieces in (S + 1, S + 2)
        assert sum(1 for x in sets[0]["buckets"] if not x.heavy and x.pieces > 1) >= 1  # unflagged buckets of several pieces
        digits.add(big.bucket)
    assert len(digits) > 32


def test_case_rows_engine():
    case = bp.case_rows_engine()
    rows = bp.nwin_for(case.c)
    (st,) = _plan(case, prepared=True, rows=rows)
    b = _by_digit(st)
    half = 1 << (case.c - 1)
    assert [(b[d].count, b[d].heavy) for d in (1, 2, 3, 4)] == [(H - 1, False), (H, False), (H + 1, True), (H, False)]
    assert (b[6].count, b[6].beg % 4, b[6].pieces, b[6].segments) == (4 * S, 0, S, 1)
    assert (b[7].count, b[7].pieces, b[7].segments) == (4 * S + 1, S + 1, 2)
    assert b[half].beg % 4 == 0 and b[half].count >= 8 * S + 1 and b[half].segments == 3 and b[half].bucket == half - 1
    # the same scalars through an unprepared handle would spread over three sets
    assert st["total"] == sum(g.count * len([d for d in bp.signed_digits(g.scalar, case.c, rows) if d])
                              for g in case.groups[0]) - 1  # (one infinity base)


def test_case_mixed_chunk():
    """eff_lgc restated: the lower sets (every scalar has a digit there) take lgc = 5, the upper ones (the short scalars
    have none) lgc = 4, and the equal scalars are a multi-segment bucket under both"""
    case = bp.case_mixed_chunk()
    nw = bp.nwin_for(case.c)
    hi, lo = bp.default_lgc(case.n)
    assert (case.n, hi, lo, nw) == (1 << 18, 5, 4, 16)
    target = bp.LANE_TARGET // nw
    sets = bp.plan(case.scalars, [True] * case.n, case.c, nw, lambda total: bp.eff_lgc(total, lo, hi, target))
    multi = {l: [s for s in sets if s["lgc"] == l and any(b.segments >= 2 for b in s["buckets"])] for l in (4, 5)}
    assert multi[4] and multi[5], [(s["total"], s["lgc"]) for s in sets]
    assert len(multi[4]) + len(multi[5]) == nw
    assert max(s["total"] for s in multi[4]) < min(s["total"] for s in multi[5])


# ---------------------------------------------------------------- the reference is right
def _points(L, n, rnd):
    g = O.G1()
    L.og1_generator(C.byref(g))
    pts = (O.G1Affine * n)()
    for i in range(n):
        t = O.G1()
        kf = O.fr_from_int(rnd.randrange(1, O.R))
        L.og1_mul(C.byref(t), C.byref(g), C.byref(kf))
        L.og1_to_affine(C.byref(pts[i]), C.byref(t))
    return pts


@pytest.fixture(scope="module")
def some_points():
    L = O.lib()
    return bytes(_points(L, 160, random.Random(404)))


SMALL = dict(H=4, S=4, C=2, c=6)
SMALL_CASES = [
    lambda: bp.case_threshold(**SMALL), lambda: bp.case_alignment(**SMALL),
    lambda: bp.case_segments(lgc=1, **SMALL), lambda: bp.case_segments_default_chunk(n=160, **SMALL),
    lambda: bp.case_segments_default_chunk(n=160, one_bin=True, **SMALL), lambda: bp.case_many_heavy(**SMALL),
    lambda: bp.case_exceptional(0, lgc=1, **SMALL), lambda: bp.case_exceptional(1, lgc=1, **SMALL),
    lambda: bp.case_exceptional(2, lgc=1, **SMALL), lambda: bp.case_exceptional(3, lgc=1, **SMALL),
    lambda: bp.case_batch3(lgc=1, **SMALL), lambda: bp.case_batch70(lgc=1, nbatch=7, **SMALL),
    lambda: bp.case_rows_engine(lgc=1, **SMALL),
]


@pytest.mark.parametrize("k", range(len(SMALL_CASES)))
def test_group_sum_reference_equals_the_oracles_pippenger(some_points, k):
    """every builder at HEAVY = HSEG = 4, chunk 2, 6-bit windows: expected() against omsm_affine on the same bases
    (repeated, negated and infinity ones included) and scalars"""
    L = O.lib()
    case = SMALL_CASES[k]()
    assert case.n <= 160
    raw = bp.materialise(case, some_points[:96 * case.n])
    pts = (O.G1Affine * case.n).from_buffer_copy(raw)
    sums = {}
    for m in range(case.nbatch):
        sc = case.scalars[m * case.n:(m + 1) * case.n]
        exp = O.G1()
        L.omsm_affine(C.byref(exp), pts, O.fr_array(sc), case.n)
        buf = C.create_string_buffer(48)
        L.og1_compress(buf, C.byref(exp))
        assert bp.expected(case.groups[m], pts, L, O, sums) == buf.raw, (case.name, m)
    # the scaled-down copy has the structure of the full one: the same groups in the same digit order, heavy where it is
    full = {c.name: c for c in bp.all_structured_cases()}[case.name]
    if case.nbatch == full.nbatch:
        assert [len(g) for g in case.groups] == [len(g) for g in full.groups]
        ps = bp.plan(case.scalars[:case.n], bp.live_mask(case), case.c, bp.nwin_for(case.c), 1, heavy=4, hseg=4,
                     prepared=case.name == "rows_engine")
        pf = _plan(full, prepared=full.name == "rows_engine")
        assert [b.heavy for b in ps[0]["buckets"]] == [b.heavy for b in pf[0]["buckets"]]


def test_exceptional_sums_are_the_stated_multiples(some_points):
    """the group sums of the +-P groups are the multiples the case states (0: infinity)"""
    L = O.lib()
    case = bp.case_exceptional(1, lgc=1, **SMALL)
    pts = (O.G1Affine * case.n).from_buffer_copy(bp.materialise(case, some_points[:96 * case.n]))
    one = lambda s: bp.Group(1, s, 0, 1)
    for g in case.groups[0]:
        kinds = case.kinds[g.start:g.start + g.count]
        if all(k == bp.DISTINCT for k in kinds):
            continue
        m = bp.exceptional_multiple(kinds)
        base = (O.G1Affine * 1).from_buffer_copy(some_points[96 * g.start:96 * g.start + 96])
        assert bp.expected([bp.Group(g.digit, 1, g.start, g.count)], pts, L, O) == bp.expected([one(m % O.R)], base, L, O), g


# ---------------------------------------------------------------- the cases tell a right engine from the two wrong ones
def _model_msm(case, msm, values, lgc, prepared, mutant):
    """The piece sums of k_accum, the two passes of k_heavy and load_bucket restated on entries — not on plan()'s formulas —
    over the integers mod r (base i stands for [values[i]] G, so the group law is addition mod r).
    mutant "a": no second pass of k_heavy; "b": the reader of a flagged bucket sums all its pieces."""
    c, n = case.c, case.n
    nw = bp.nwin_for(c)
    sc = case.scalars[msm * n:(msm + 1) * n]
    sets = [[] for _ in range(1 if prepared else nw)]
    for i, s in enumerate(sc):
        if case.kinds[i] == bp.INF or not s:
            continue
        for w, d in enumerate(bp.signed_digits(s, c, nw)):
            if d:
                v = values[i] << (c * w) if prepared else values[i]
                sets[0 if prepared else w].append((abs(d) - 1, v if d > 0 else -v))
    total = 0
    for w, ent in enumerate(sets):
        ent.sort(key=lambda e: e[0])
        slots, first, last, count = {}, {}, {}, {}
        for k, (b, v) in enumerate(ent):
            t = k >> lgc
            slots[(b, t)] = slots.get((b, t), 0) + v  # k_accum: the piece of bucket b inside chunk t
            first.setdefault(b, t)
            last[b] = t
            count[b] = count.get(b, 0) + 1
        wsum = 0
        for b in count:
            t0, t1 = first[b], last[b]
            flagged = count[b] > H
            if flagged:
                pieces = t1 - t0 + 1
                for k0 in range(0, pieces, S):  # pass 1: HSEG consecutive pieces into the segment's first slot
                    slots[(b, t0 + k0)] = sum(slots[(b, t0 + k)] for k in range(k0, min(k0 + S, pieces)))
                if mutant != "a":                # pass 2: the segment sums into the bucket's first slot
                    slots[(b, t0)] = sum(slots[(b, t0 + k0)] for k0 in range(0, pieces, S))
            if flagged and mutant != "b":
                val = slots[(b, t0)]
            else:
                val = sum(slots[(b, t)] for t in range(t0, t1 + 1))
            wsum += (b + 1) * val
        total += wsum if prepared else wsum << (c * w)
    return total % bp.R


@pytest.mark.parametrize("name", [c.name for c in bp.all_structured_cases()])
def test_each_case_tells_the_engine_from_its_mutants(name):
    """at the engine's own constants: the restated pipeline gives sum s_i k_i for every case; without k_heavy's second
    pass it is wrong exactly for the MSMs whose plan has a bucket of more than HSEG pieces, and with a reader that ignores
    the heavy flag exactly for those with a flagged bucket of two or more pieces — what the two mutants of the library
    must show on the GPU (profiles/NOTES.md §28)"""
    case = {c.name: c for c in bp.all_structured_cases()}[name]
    rnd = random.Random(len(name))
    values = [rnd.randrange(1, bp.R) for _ in range(case.n)]
    for i, k in enumerate(case.kinds):
        if k == bp.INF:
            values[i] = 0
        elif k != bp.DISTINCT:
            values[i] = values[k[1]] if k[0] == bp.REPEAT else -values[k[1]]
    prepared = name == "rows_engine"
    lgc = case.lgc if case.lgc is not None else bp.default_lgc(case.n)[0]
    fails = {"a": 0, "b": 0}
    for m in range(0, case.nbatch, 1 if case.nbatch <= 3 else 9):  # (the seventy MSMs differ in their digits only)
        sc = case.scalars[m * case.n:(m + 1) * case.n]
        want = sum(s * v for s, v in zip(sc, values)) % bp.R
        assert _model_msm(case, m, values, lgc, prepared, None) == want
        sets = _plan(case, msm=m, prepared=prepared, rows=bp.nwin_for(case.c) if prepared else None)
        predicted = {"a": any(b.segments >= 2 for s in sets for b in s["buckets"]),
                     "b": any(b.heavy and b.pieces >= 2 for s in sets for b in s["buckets"])}
        for mut in "ab":
            wrong = _model_msm(case, m, values, lgc, prepared, mut) != want
            assert wrong == predicted[mut], (name, m, mut)
            fails[mut] += wrong
    assert fails["b"] >= 1  # every case has a flagged bucket of several pieces
    assert (fails["a"] >= 1) == (name not in ("threshold", "alignment", "many_heavy"))
