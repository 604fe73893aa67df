"""The lazy Fr arithmetic of the NTT kernels (fr29.hip.h) and the lane scan of frscan.hip.h on the device, at the bounds
the headers state, against the Python-integer checkers of tests/fr29_cases.py.

tests/device_checks/fr_check.hip is compiled with the product's compiler and flags (rust-kzg_amd/build.py) once per
define set — the product's form and -DFR_CHECK_UNCHAINED (mul_signed without the opaque accumulator chain) — and every
build is held to the checkers, not to another build.  The module needs no library, so it does not take the `kzg` fixture
and runs once.

A harness run is one child process with a time limit; one is alive at a time.  If one ends abnormally — a signal, a
timeout, a non-zero exit, an error line — the module records that and every later test of the module skips with the
reason: nothing is run again on a device that has just faulted.

The last test builds the harness with -DFR_CHECK_PLANT_ERROR, which adds 1 to one word of the result of case 1 of every
op, and asserts that the checkers object to exactly those cases."""
import subprocess

import pytest

import fr29_cases as F
import lane_harness as H

pytestmark = pytest.mark.gpu

RUN_TIMEOUT = 120  # seconds for one harness run (a second or two when all is well)
_abnormal = []     # why the first abnormal harness run ended; set once

MUL_OPS = ("msig", "msig2", "mul", "mulb", "twist")
BUTTERFLY_OPS = ("bfs", "bfl", "bfl8", "round", "round_unit")
REDUCE_OPS = ("redl", "fin", "pack", "unpack", "unpack_shl5")


@pytest.fixture(scope="module")
def cases():
    """(cases, cross-checks): every op of the host test, the new ops and the scan"""
    c, cross = F.all_cases()
    c = c + F.scan_cases()
    per_op = {}
    for op, _, _ in c:
        per_op[op] = per_op.get(op, 0) + 1
    assert set(per_op) == set(MUL_OPS + BUTTERFLY_OPS + REDUCE_OPS + ("scan",)) == set(F.SHAPES)
    print("Fr arithmetic cases per op:", ", ".join("%s %d" % kv for kv in per_op.items()), "- total", len(c))
    return c, cross


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """every build of the harness, compiled side by side into a temporary directory (hipcc only: no GPU process yet)"""
    sets = dict(H.FR_DEFINE_SETS)
    sets.update(H.FR_PLANTED)
    built, errors = H.compile_all(tmp_path_factory.mktemp("fr_check"), sets, H.FR_SOURCE)
    assert not errors, "hipcc failed on the harness: %s" % errors
    return built


@pytest.fixture(scope="module", params=list(H.FR_DEFINE_SETS))
def harness(request, builds):
    return builds[request.param]


def run_harness(exe, cases):
    """one child process, one time limit; returns its output.  An abnormal end is recorded and fails the test; after
    one, every call skips."""
    if _abnormal:
        pytest.skip("an earlier harness run ended abnormally (%s): nothing more runs on the device" % _abnormal[0])
    why = None
    out = ""
    try:
        p = subprocess.run([exe], input=F.encode(cases), capture_output=True, text=True, timeout=RUN_TIMEOUT)
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
    return out


def check(exe, cases, ops):
    allc, cross = cases
    keep = [i for i, c in enumerate(allc) if c[0] in ops]
    pos = {i: k for k, i in enumerate(keep)}
    mine = [allc[i] for i in keep]
    mycross = [tuple(pos[i] for i in c) for c in cross if all(i in pos for i in c)]
    bad = F.failures(mine, run_harness(exe, mine), mycross)
    assert not bad, "%d of %d cases fail, the first: %s" % (len(bad), len(mine), bad[:4])


def test_multipliers_at_their_bounds(harness, cases):
    """mul_signed (multiplicand in (-r, 64r) with limbs up to 1.5 * 2^30 and a signed top limb, products that are small
    residues: result just above -r), mul_signed2 (an edge pair next to an ordinary one, each pair also alone through
    mul_signed: limb for limb the same), mul, mul_blst (0, 1, r - 1, 2^256 - 1 and the largest pairs with
    a * b < 2^256 r: result in [0, r)), the DAS twist (0 < value < 2r, normalised)"""
    check(harness, cases, MUL_OPS)


def test_butterflies_and_rounds_at_their_bounds(harness, cases):
    """butterfly_signed / butterfly_lazy / butterfly_lazy8 (value identities, no limb wraps), a round of four butterflies
    with one carry pass, and a transform's first round as ntt_round chains it, on canonical inputs and inputs up to
    2^256 - 1 (normalised, never negative, grown by < 13r)"""
    check(harness, cases, BUTTERFLY_OPS)


def test_reductions_and_bit_reslicing(harness, cases):
    """reduce_lazy on EVERY multiple of r below 64r and its neighbours, finish on the same operands, pack / unpack round
    trips, unpack_shl5(a) = 32 a for a up to 2^256 - 1"""
    check(harness, cases, REDUCE_OPS)


def test_scan_suffix_for_every_group_width(harness, cases):
    """scan_suffix for gw = 1, 2, 4, ..., 64 with a different C per case, S = 0, r - 1 or random per lane and idle lanes
    carrying zeros: every lane against sum C^d S"""
    check(harness, cases, ("scan",))


def test_planted_errors_are_found_exactly(builds, cases):
    """-DFR_CHECK_PLANT_ERROR: one word of the result of case 1 of every op is off by one; the checkers must object to
    those cases and to no other"""
    allc, cross = cases
    flagged = {(op, i) for op, i, _ in F.failures(allc, run_harness(builds["planted"], allc), cross)}
    want = {(op, 1) for op in F.SHAPES}
    assert flagged == want, (sorted(flagged - want), sorted(want - flagged))
