"""The variable-base MSM engine at its bucket-size and segment edges (tests/bucket_plan.py builds the cases, the CPU module
test_msm_bucket_edges_cpu.py proves that each contains the edge it is named after): buckets of exactly HEAVY - 1, HEAVY and
HEAVY + 1 entries, buckets of exactly HSEG, HSEG + 1 and 2 HSEG + 1 pieces (the second pass of k_heavy), every
alignment of a bucket against the chunks of k_accum, heavy buckets in the first and the last bucket of a set, more heavy
buckets than k_heavy's first pass has workgroups, equal / opposite / infinity bases inside a heavy bucket, batches on both
sides of the 64-set limit, the rows engine's one shared set, and a launch whose sets took different chunks.

The endomorphism split is off (glv=0) and the window forced, so that a scalar d * (1 + 2^c + ... + 2^(c (J-1))) is an
entry of bucket d - 1 in each of the first J sets; the expected value is sum_j [s_j] (sum of the points of group j) on the
oracle's point arithmetic — no Pippenger anywhere in the reference.  Every result is compared by its compressed bytes."""
import ctypes as C

import pytest

import bucket_plan as bp
import oracle_ffi as O

pytestmark = pytest.mark.gpu

# forms of the engine (tuning keys added to the steering ones); keys an entry point ignores at a size change nothing
ALL_FORMS = [{}, {"one_level_sort": 1}, {"direct_scatter": 1}, {"scatter_atomics": 1}, {"no_wide_tail": 1}, {"tree_tail": 1},
             {"digit_min_log": 10}, {"digit_min_log": 10, "flat_digits": 1}]
TWO_FORMS = [{}, {"digit_min_log": 10}]  # the (A, M) tree with load_bucket, and the tiled digit reduction

CASES = {
    "threshold": bp.case_threshold, "alignment": bp.case_alignment, "segments": bp.case_segments,
    "segments_default_chunk": bp.case_segments_default_chunk,
    "segments_default_chunk_one_bin": lambda: bp.case_segments_default_chunk(one_bin=True),
    "many_heavy": bp.case_many_heavy,
    "exceptional_0": lambda: bp.case_exceptional(0), "exceptional_1": lambda: bp.case_exceptional(1),
    "exceptional_2": lambda: bp.case_exceptional(2), "exceptional_3": lambda: bp.case_exceptional(3),
    "batch3": bp.case_batch3, "batch70": bp.case_batch70, "rows_engine": bp.case_rows_engine, "mixed_chunk": bp.case_mixed_chunk,
}
_prepared = {}  # case name -> (case, bases, scalars, expected compressed result per MSM): built once, never changed


def _compressed(L, raw144):
    g = O.G1()
    C.memmove(C.byref(g), raw144, 144)
    buf = C.create_string_buffer(48)
    L.og1_compress(buf, C.byref(g))
    return buf.raw


def _case(name, kzg, L):
    """the case, its bases (generated on the device, copied back once, the repeated / negated / infinity ones written over
    them on the host), its scalars and the reference"""
    if name in _prepared:
        return _prepared[name]
    import torch

    case = CASES[name]()
    stream = torch.cuda.current_stream().cuda_stream
    d_pts = torch.empty(case.n * 96, dtype=torch.uint8, device="cuda")
    kzg.generate_points(d_pts.data_ptr(), case.n, 90 + list(CASES).index(name), stream)
    torch.cuda.synchronize()
    raw = bp.materialise(case, d_pts.cpu().numpy().tobytes())
    pts = (O.G1Affine * case.n).from_buffer_copy(raw)
    sc = bp.scalar_bytes(case)
    if name == "mixed_chunk":
        exp = O.G1()
        L.omsm_tiling_pippenger(C.byref(exp), pts, sc, case.n)
        want = [_compressed(L, bytes(exp))]
    else:
        sums = {}
        want = [bp.expected(case.groups[m], pts, L, O, sums) for m in range(case.nbatch)]
    _prepared[name] = (case, raw, sc, want)
    return _prepared[name]


def _run(kzg, L, name, form, rows_engine=False):
    import torch

    case, raw, sc, want = _case(name, kzg, L)
    stream = torch.cuda.current_stream().cuda_stream
    tuning = {"window_prepared": case.c} if rows_engine else {"glv": 0, "window": case.c}
    if case.lgc is not None:
        tuning["lgc"] = case.lgc
    tuning.update(form)
    if rows_engine:
        pts = (O.G1Affine * case.n).from_buffer_copy(raw)
        h = kzg.prepare_multi_scalar_mult(pts, case.n, kzg.make_config(no_tables=True, tuning=tuning))
        assert not h.info()["wide_table"]
    else:
        d_pts = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
        h = kzg.DeviceMsm(d_pts.data_ptr(), case.n, False, kzg.make_config(tuning=tuning))
    assert h.info()["window_bits"] == case.c, h.info()
    d_sc = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
    d_out = torch.ones(144 * case.nbatch, dtype=torch.uint8, device="cuda")
    kzg.msm_prepared_batch_device(h, d_out.data_ptr(), d_sc.data_ptr(), case.n, case.nbatch, False, stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().tobytes()
    h.close()
    got = [_compressed(L, out[144 * m:144 * m + 144]) for m in range(case.nbatch)]
    wrong = [m for m in range(case.nbatch) if got[m] != want[m]]
    assert not wrong, (name, form, wrong)
    return got


def _id(form):
    return ",".join("%s=%d" % kv for kv in form.items()) or "default"


@pytest.mark.parametrize("form", ALL_FORMS, ids=_id)
@pytest.mark.parametrize("name", ["segments", "segments_default_chunk", "segments_default_chunk_one_bin"])
def test_segments_of_a_heavy_bucket(oracle, kzg, name, form):
    """buckets of exactly HSEG, HSEG + 1 and 2 HSEG + 1 pieces, and HSEG + 1 pieces from HSEG chunks' worth of entries that
    begin one entry after a chunk start — with 4-entry chunks through the one-level sort (segments), with the default
    16-entry chunks through the two-level sort at n = 2^15 — under every form of the engine"""
    _run(kzg, oracle.lib(), name, form)


@pytest.mark.parametrize("form", TWO_FORMS, ids=_id)
@pytest.mark.parametrize("name", ["threshold", "alignment", "many_heavy"])
def test_heavy_threshold_and_piece_geometry(oracle, kzg, name, form):
    """threshold: buckets of HEAVY - 1, HEAVY, HEAVY + 1 entries and one of HEAVY + 1 bases of which one is infinity;
    alignment: heavy buckets beginning 1 and chunk - 1 entries after a chunk start with a last piece of one entry, ending
    exactly at a chunk end, and in the last bucket of the set; many_heavy: 264 heavy buckets in one launch"""
    _run(kzg, oracle.lib(), name, form)


@pytest.mark.parametrize("form", TWO_FORMS, ids=_id)
@pytest.mark.parametrize("rot", range(4))
def test_exceptional_additions_inside_heavy_buckets(oracle, kzg, rot, form):
    """the heavy buckets of `segments` filled with one repeated point, with P and -P in equal numbers (the bucket is
    infinity), with a surplus of three, and with infinity bases among them: k_accum's chain doubles and cancels mid-chain,
    k_heavy's tree adds equal pieces, opposite pieces and infinities"""
    L = oracle.lib()
    got = _run(kzg, L, "exceptional_%d" % rot, form)
    assert got[0] != b"\xc0" + bytes(47)


@pytest.mark.parametrize("form", TWO_FORMS, ids=_id)
@pytest.mark.parametrize("name", ["batch3", "batch70"])
def test_heavy_buckets_in_a_batch(oracle, kzg, name, form):
    """one handle, several MSMs in one call: three (60 bucket sets: `segments`, all-zero scalars, one scalar for all
    points) and seventy (more than 64 sets: k_level<true> reads the heavy flags through load_bucket)"""
    L = oracle.lib()
    got = _run(kzg, L, name, form)
    if name == "batch3":
        assert got[1] == b"\xc0" + bytes(47)


@pytest.mark.parametrize("form", TWO_FORMS, ids=_id)
def test_heavy_buckets_in_the_rows_engine(oracle, kzg, form):
    """a prepared handle without a wide table: all windows share one bucket set, and m points with J non-zero digits are
    m J entries of one bucket — across HEAVY, HSEG chunks and 2 HSEG chunks"""
    _run(kzg, oracle.lib(), "rows_engine", form, rows_engine=True)


@pytest.mark.parametrize("form", TWO_FORMS, ids=_id)
def test_heavy_bucket_in_sets_of_different_chunks(oracle, kzg, form):
    """n = 2^18: the upper sets hold half as many entries as the lower ones and take 16-entry chunks instead of 32-entry
    ones; 32 769 equal scalars are a two-segment bucket in every set under either chunk (the oracle's Pippenger is the
    reference here: the scalars are random)"""
    _run(kzg, oracle.lib(), "mixed_chunk", form)
