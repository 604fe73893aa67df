"""The lane-parallel Fp and G1 arithmetic (fpw.hip.h, g1w.hip.h, g1grp.hip.h) on the device, at the bounds its
headers state, against the Python-integer model of tests/lane_model.py.

tests/device_checks/lane_check.hip is compiled with the product's compiler and flags (rust-kzg_amd/build.py) once per
define set — the product's, -DKZGAMD_FORCE_EXACT_TESTS (no filter in front of the exact zero test) and
-DKZGAMD_WMUL_DIGIT_AHEAD (the other digit computation of wmul4) — and every build is held to the model, not to
another build.  The module needs no library, so it does not take the `kzg` fixture and runs once.

A harness run is one child process with a time limit; one is alive at a time.  If one ends abnormally — a signal, a
timeout, a non-zero exit, an error line — the module records that and every later test of the module skips with the
reason: nothing is run again on a device that has just faulted.

The last test builds the harness with -DLANE_CHECK_PLANT_ERROR, which adds 1 to one limb of the result of case 1 of
every op, and asserts that the checkers object to exactly those cases."""
import subprocess

import pytest

import lane_harness as H
import lane_model as M

pytestmark = pytest.mark.gpu

RUN_TIMEOUT = 120  # seconds for one harness run (a second or two when all is well)
_abnormal = []     # why the first abnormal harness run ended; set once

FPW_OPS = ("wnorm", "wnorm_full", "waddn", "wsub16", "wsub32", "wmul4", "wsqr", "wdbl", "wide_roundtrip")
G1W_OPS = ("load_store", "is_zero", "dbl", "dadd", "dbl_k", "add_n")
GRP_OPS = ("grp_dbl1", "grp_dbl2", "grp_dbl4", "grp_dadd1", "grp_dadd2", "grp_dadd4", "grp_madd4")
ONE_OPS = ("one_dadd", "one_dadd_unequal", "one_dbl_k", "one_to_blst", "one_reduce_xy", "one_madd", "one_chain_add")


@pytest.fixture(scope="module")
def blocks():
    b = M.all_cases()
    assert set(b) == set(FPW_OPS + G1W_OPS + GRP_OPS + ONE_OPS + ("chain",))
    print("lane arithmetic cases per op:", ", ".join("%s %d" % (op, len(v)) for op, v in b.items()), "- total",
          sum(len(v) for v in b.values()))
    return b


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """every build of the harness, compiled side by side into a temporary directory (hipcc only: no GPU process yet)"""
    sets = dict(H.DEFINE_SETS)
    sets.update(H.PLANTED)
    built, errors = H.compile_all(tmp_path_factory.mktemp("lane_check"), sets)
    assert not errors, "hipcc failed on the harness: %s" % errors
    return built


@pytest.fixture(scope="module", params=list(H.DEFINE_SETS))
def harness(request, builds):
    return builds[request.param]


def run_harness(exe, blocks):
    """one child process, one time limit; returns op -> outputs.  An abnormal end is recorded and fails the test; after
    one, every call skips."""
    if _abnormal:
        pytest.skip("an earlier harness run ended abnormally (%s): nothing more runs on the device" % _abnormal[0])
    why = None
    out = ""
    try:
        p = subprocess.run([exe], input=M.encode(blocks), capture_output=True, text=True, timeout=RUN_TIMEOUT)
        out = p.stdout
        if p.returncode < 0:
            why = "signal %d" % -p.returncode
        elif p.returncode != 0:
            why = "exit status %d: %s" % (p.returncode, (p.stdout[-300:] + p.stderr[-300:]).strip())
        elif "error" in p.stdout[-2000:] or "HIP error" in p.stderr:
            why = "error line: %s" % (p.stdout[-300:] + p.stderr[-300:]).strip()
    except subprocess.TimeoutExpired:
        why = "no end after %d s" % RUN_TIMEOUT
    if why:
        _abnormal.append(why)
        pytest.fail("harness run ended abnormally: " + why)
    return M.decode(out, blocks)


def check(exe, blocks, ops):
    mine = {op: blocks[op] for op in ops}
    outs = run_harness(exe, mine)
    bad = M.failures(mine, outs)
    assert not bad, "%d of %d cases fail, the first: %s" % (len(bad), sum(len(v) for v in mine.values()), bad[:6])
    return outs


def test_fpw_primitives_at_their_bounds(harness, blocks):
    """wnorm / wnorm_full (value unchanged, limbs <= 2^28 / < 2^28, from limbs up to 2^31 - 1 and the longest carry
    ripple), waddn / wsub16 / wsub32 (value identities with b wide-normal up to just under 15p / 31p: no limb wraps),
    wmul4 / wsqr (residue, value < 2p, limbs <= 2^28 for operands with limbs < 2^29 up to the product bound), wdbl (its
    invariant holds again), to_wide -> from_wide; four different inputs in the four rows of a wave, lanes 14 and 15 of
    every row zero in every result"""
    check(harness, blocks, FPW_OPS)


def test_wmul4_rows_depend_on_their_own_operands_only(harness):
    """four different pairs, each alone and all at once in each rotation of the rows: limb for limb the same results"""
    import random

    cases, cross_check = M.wmul_row_independence(random.Random(4))
    mine = {"wmul4": cases}
    outs = run_harness(harness, mine)
    assert not M.failures(mine, outs)
    cross_check(outs["wmul4"])


def test_g1w_point_operations_and_every_exceptional_case(harness, blocks):
    """load / store / to_single (exactly normalized, 56 words and no more), is_zero_mod_p (every k*p, k < 64, its
    neighbours and the non-multiples that pass the filter: the same answers with and without the filter), dbl, dadd with
    infinity on either side, P + P and P + (-P) in equal and different representations, dbl_k for k in 0, 1, 2, 5, 64,
    add_n for n = 1..5 and strides 1 and 3 through infinity and through a doubling: the represented point, ZZ^3 = ZZZ^2,
    X, Y < 18p, ZZ, ZZZ < 2p, limbs <= 2^28, the four rows identical, lanes 14 and 15 zero"""
    check(harness, blocks, G1W_OPS)


def test_g1w_chains_keep_their_bounds_step_by_step(harness, blocks):
    """scripted chains of 64 mixed dbl / dadd / dbl_k steps: the bounds and the point after every step"""
    check(harness, blocks, ("chain",))


def test_lane_group_bodies_on_every_group_position(harness, blocks):
    """grp::dbl_body<G>, dadd_body<G> (G = 1, 2, 4) and madd_body4 at the bounds of g1::dbl / dadd / madd, different cases
    — exceptional next to ordinary — in the groups of one wave, every case on every group position of a quad: every lane
    of a group holds the same result, the flag of dadd_body is set exactly for P + P"""
    check(harness, blocks, GRP_OPS)


def test_single_lane_routines_on_wide_stored_points(harness, blocks):
    """the single-lane consumers of arrays the wide kernels store into, on points with X, Y just under 18p (DESIGN.md,
    the boundary table); madd and chain_add, which never read such points, at their own bounds"""
    check(harness, blocks, ONE_OPS)


def test_planted_errors_are_found_exactly(builds, blocks):
    """-DLANE_CHECK_PLANT_ERROR: one limb of the result of case 1 of every op is off by one; the checkers must object
    to those cases and to no other"""
    outs = run_harness(builds["planted"], blocks)
    flagged = {(op, i) for op, i, _ in M.failures(blocks, outs)}
    assert flagged == {(op, 1) for op in blocks}, (sorted(flagged - {(op, 1) for op in blocks}), sorted({(op, 1) for op in blocks} - flagged))
