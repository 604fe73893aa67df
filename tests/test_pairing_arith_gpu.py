"""The pairing tower of fp12w.hip.h on the device — every operation of the interpreter, the Miller loop and the final
exponentiation, one wave per case — against the Python-integer model of tests/pairing_model.py, value for value.

tests/device_checks/pairing_check.hip is compiled with the product's compiler and flags (rust-kzg_amd/build.py), for
the product's defines and for -DKZGAMD_FORCE_EXACT_TESTS (no filter in front of the exact zero tests of the verdict and
of the Z = 0 test), and both builds are held to the model, not to each other.  The module needs no library, so it does
not take the `kzg` fixture.

A harness run is one child process with a time limit; one is alive at a time.  If one ends abnormally — a signal, a
timeout, a non-zero exit, an error line — the module records that and every later test of the module skips with the
reason: nothing is run again on a device that has just faulted.

The last test builds the harness with -DPAIRING_CHECK_PLANT_ERROR, which adds 1 to one limb of the result of case 1 of
every block, and asserts that the checkers object to exactly those cases."""
import os
import random
import subprocess

import pytest

import lane_harness as H
import pairing_model as M

pytestmark = pytest.mark.gpu

SOURCE = os.path.join(H.HERE, "device_checks", "pairing_check.hip")
DEFINE_SETS = {"product": [], "exact": ["-DKZGAMD_FORCE_EXACT_TESTS"]}
PLANTED = {"planted": ["-DPAIRING_CHECK_PLANT_ERROR"]}
RUN_TIMEOUT = 120  # seconds for one harness run (about a second when all is well)
_abnormal = []     # why the first abnormal harness run ended; set once


@pytest.fixture(scope="module")
def blocks():
    """computed once and left unchanged: a few dozen cases per operation and 8 full checks"""
    b = {"unit": M.unit_cases(random.Random(2024), per_op=24), "pairing": M.pairing_cases(), "winv": M.winv_cases(random.Random(50))}
    print("pairing arithmetic cases:", ", ".join("%s %d" % (op, len(v)) for op, v in b.items()))
    return b


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    sets = dict(DEFINE_SETS)
    sets.update(PLANTED)
    built, errors = H.compile_all(tmp_path_factory.mktemp("pairing_check"), sets, SOURCE)
    assert not errors, "hipcc failed on the harness: %s" % errors
    return built


@pytest.fixture(scope="module", params=list(DEFINE_SETS))
def harness(request, builds):
    return builds[request.param]


def run_harness(exe, blocks):
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


def test_every_tower_operation_at_its_bounds(harness, blocks):
    """f12_mul, f12_sqr, f12_cyclotomic_sqr, f12_conj, f12_frobenius, f12_inv and the line step (both pairs, either or
    both skipped): operands random, at the upper bound of the value (2p - 1) and of the limbs (2^28), zero, one, and
    0 mod p as p in limb form.  Every result register holds exactly the model's integer in all four rows, limbs <= 2^28,
    lanes 14 and 15 zero, value < 2p."""
    mine = {"unit": blocks["unit"]}
    outs = run_harness(harness, mine)
    bad = M.failures(mine, outs)
    assert not bad, "%d of %d cases fail, the first: %s" % (len(bad), len(mine["unit"]), bad[:6])


def test_miller_loop_final_exponentiation_and_verdicts(harness, blocks):
    """8 checks from blst_p1 inputs and two line tables: the value of slot 0 after the program, the skipped pairs and
    the verdict — true, false, Z != 1, infinity, an identity G2 point, a point outside G1, the Miller loop alone"""
    mine = {"pairing": blocks["pairing"]}
    outs = run_harness(harness, mine)
    bad = M.failures(mine, outs)
    assert not bad, bad[:6]


def test_the_fp_inversion_alone(harness, blocks):
    """winv at zero, 0 mod p as p and as 49p, one, just under its bound of 50p, with limbs at 2^28, and random values"""
    mine = {"winv": blocks["winv"]}
    outs = run_harness(harness, mine)
    bad = M.failures(mine, outs)
    assert not bad, bad[:6]


def test_planted_errors_are_found_exactly(builds, blocks):
    outs = run_harness(builds["planted"], blocks)
    flagged = {(op, i) for op, i, _ in M.failures(blocks, outs)}
    assert flagged == {(op, 1) for op in blocks}, sorted(flagged)
