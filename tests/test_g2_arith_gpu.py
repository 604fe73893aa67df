"""The Fp2 and G2 arithmetic that holds one value per lane (g2_28.hip.h, g2_io.hip.h, g2_lincomb.hip.h) and the
fp28.hip.h primitives under it, on the device, at the bounds the headers state, against the Python-integer model of
tests/g2_lane_cases.py.  The host build of the same text is checked on the CPU (test_g2_lane_cpu.py, test_g2_add_cpu.py,
test_point_codec_cpu.py, test_host_cpu.py, test_g2_device_cases_cpu.py); this module is where the device build —
v_mad_u64_u32 column chains, the register allocation of large kernels under __launch_bounds__(64), 64 lanes in
different cases of one addition at once — is held to the same tables, routine by routine.

tests/device_checks/g2_check.hip is compiled with the product's compiler and flags (rust-kzg_amd/build.py) once per
define set — the product's and -DKZGAMD_FORCE_EXACT_TESTS (no filter in front of the exact zero test) — and every build
is held to the model, not to another build.  The module needs no library, so it does not take the `kzg` fixture.

A harness run is one child process with a time limit; one is alive at a time.  If one ends abnormally — a signal, a
timeout, a non-zero exit, an error line — the module records that and every later test of the module skips with the
reason: nothing is run again on a device that has just faulted, and nothing is tried twice.

One test per layer and build, so that a failure names its layer: fp, fp2, the point routines with every wave mixed and
with whole waves of one exceptional kind, g2io, g2lc mixed and uniform.  The last test runs the build with
-DG2_CHECK_PLANT_ERROR, which spoils the result of case 1 of every block, and asserts that the checkers object to
exactly those cases."""
import subprocess
import time

import pytest

import g2_lane_cases as G
import lane_harness as H
from test_lane_arith_gpu import RUN_TIMEOUT

pytestmark = pytest.mark.gpu

_abnormal = []  # why the first abnormal harness run ended; set once


@pytest.fixture(scope="module")
def blocks():
    b = G.all_cases()
    per_op = G.cases_per_op(b)
    print("G2 lane arithmetic cases per op:", ", ".join("%s %d" % kv for kv in per_op.items()), "- total", sum(per_op.values()))
    return b


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """every build of the harness, compiled side by side into a temporary directory (hipcc only: no GPU process yet)"""
    sets = dict(H.G2_DEFINE_SETS)
    sets.update(H.G2_PLANTED)
    built, errors = H.compile_all(tmp_path_factory.mktemp("g2_check"), sets, H.G2_SOURCE)
    assert not errors, "hipcc failed on the harness: %s" % errors
    return built


@pytest.fixture(scope="module", params=list(H.G2_DEFINE_SETS))
def harness(request, builds):
    return builds[request.param]


def run_harness(exe, blocks):
    """one child process, one time limit; returns block -> outputs.  An abnormal end is recorded and fails the test;
    after one, every call skips."""
    if _abnormal:
        pytest.skip("an earlier harness run ended abnormally (%s): nothing more runs on the device" % _abnormal[0])
    why = None
    out = ""
    began = time.time()
    try:
        p = subprocess.run([exe], input=G.encode(blocks), capture_output=True, text=True, timeout=RUN_TIMEOUT)
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
    print("harness run: %d cases in %.1f s" % (sum(len(v) for v in blocks.values()), time.time() - began))
    return G.decode(out, blocks)


def check(exe, blocks, layer):
    mine = {b: blocks[b] for b in G.LAYERS[layer]}
    outs = run_harness(exe, mine)
    bad = G.failures(mine, outs)
    assert not bad, "%d of %d cases fail, the first: %s" % (len(bad), sum(len(v) for v in mine.values()), bad[:6])


def test_fp28_primitives_at_their_bounds(harness, blocks):
    """mul / sqr / mul2_inline (30-bit limbs, both operands lazy in the low half, the 2^63 column bound), sub<K> /
    sub_lazy<K> / neg<K> for every pad, sub_signed_lazy<8|16> with both masks and s, y at their maxima (no limb wraps,
    the top limb never negative), sub_2b_c, norm, is_zero_mod_p on every multiple below 64p, its neighbours, lazy sums
    and the values that pass the filter, canon, the blst conversions"""
    check(harness, blocks, "fp")


def test_fp2_routines_at_the_top_of_their_table(harness, blocks):
    """every row of g2_28.hip.h's Fp2 table: a residue plus (K - 1) p on every component, the limb patterns, k p and
    its neighbours; exact values for add / dbl / sub / neg, residues and the stated output bounds for the products"""
    check(harness, blocks, "fp2")


def test_g2_point_routines_in_mixed_waves(harness, blocks):
    """dbl, madd (with its state), madd_complete, madd_tab and add with every exceptional kind next to generic cases in
    every wave; the outputs of dbl, madd and add fed into each of them; to_affine and the blst_p2 conversions"""
    check(harness, blocks, "g2_mixed")


def test_g2_point_routines_in_uniform_waves(harness, blocks):
    """whole waves of 64 x P + P, 64 x P - P, 64 x infinity + P, 64 flagged table entries"""
    check(harness, blocks, "g2_uniform")


def test_g2_wire_format_and_membership(harness, blocks):
    """canon2, lex_largest, sqrt with 63p on top of the components, every catalogued encoding through uncompress,
    in_g2 and compress, psi and its constants as the device holds them"""
    check(harness, blocks, "g2io")


def test_g2_lincomb_term_and_tree_in_mixed_waves(harness, blocks):
    """g2lc::term for every scalar case, neighbours in a wave with scalars of 0 to 255 bits, the order-13 point and
    identities; tree_step for one level and for all six, the 64 slots in LDS"""
    check(harness, blocks, "g2lc_mixed")


def test_g2_lincomb_term_in_uniform_waves(harness, blocks):
    """64 zero scalars, 64 identities, 64 multiples of 13 over the order-13 point, 64 scalars just below r"""
    check(harness, blocks, "g2lc_uniform")


def test_planted_errors_are_found_exactly(builds, blocks):
    """-DG2_CHECK_PLANT_ERROR: one limb, verdict or byte of the result of case 1 of every block is off; the checkers
    must object to those cases and to no other"""
    outs = run_harness(builds["planted"], blocks)
    flagged = {(b, i) for b, i, _ in G.failures(blocks, outs)}
    want = {(b, 1) for b in blocks}
    assert flagged == want, (sorted(flagged - want), sorted(want - flagged))
