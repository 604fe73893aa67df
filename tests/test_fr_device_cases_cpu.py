"""What the GPU tests of the Fr arithmetic rest on, checked without a GPU: tests/device_checks/fr_check.hip cross-compiles
for gfx950 in every define set; the ops it adds to the host test's pass on a host build of the same headers (and a
planted error is found exactly); the lazy-pass model (tests/ntt_lazy_model.py) returns the residues of a plain
transform at every shape the stored worst-case vectors use; every stored vector (tests/golden/ntt_worst_inputs.json)
reaches its recorded value through the model, and that value is where the issue wants it:

  * the forward 4096-point vector aimed at output 4095 reaches at least 57r;
  * every aimed vector comes within 4r of its path bound (ntt_lazy_model.path_bound: x0 + 4r + 5r (T - 1) for the last
    output of a first pass, x0 + 5r T in a later pass; the deficit is sum a_s W_s / 2^261 < 3.7r for twelve stages);
  * every aimed vector exceeds the maximum over three random vectors of the same shape by at least 3r — where that is
    possible at all: a pass of T <= 7 stages has its bound (30r, 35r, 36r) less than 3r above what random inputs reach
    (27.0r, 32.6r, 33.6r), so no input can; those vectors are held to 1r below their path bound instead, and above random;
  * no value anywhere in any run reaches 64r."""
import json
import os
import random
import shutil
import subprocess

import pytest

import fr29_cases as F
import lane_harness as H
import ntt_lazy_model as M

R = M.R
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ntt_worst_inputs.json")


# ------------------------------------------------------------------------------------------------ the harness
@pytest.fixture(scope="module")
def cross_compiled(tmp_path_factory):
    if not os.path.exists(H.product_build().hipcc_path()):
        pytest.skip("no hipcc on this machine")
    sets = dict(H.FR_DEFINE_SETS)
    sets.update(H.FR_PLANTED)
    return H.compile_all(tmp_path_factory.mktemp("fr_check"), sets, H.FR_SOURCE)


@pytest.mark.parametrize("name", list(H.FR_DEFINE_SETS) + list(H.FR_PLANTED))
def test_fr_harness_cross_compiles_for_gfx950(cross_compiled, name):
    """a header change that breaks tests/device_checks/fr_check.hip shows here, on a machine without a GPU"""
    built, errors = cross_compiled
    assert name in built, errors.get(name)
    cmd = H.compile_command("x", H.FR_DEFINE_SETS.get(name, H.FR_PLANTED.get(name)), H.FR_SOURCE)
    assert "--offload-arch=gfx950" in cmd and "-O3" in cmd and "-std=c++17" in cmd and H.FR_SOURCE in cmd


@pytest.fixture(scope="module")
def host_builds(tmp_path_factory):
    """fr_check.hip's host form (-DFR_CHECK_HOST): the same run_case() over the same headers, no HIP"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    d = tmp_path_factory.mktemp("fr_check_host")
    out = {}
    for name, defines in (("product", []), ("unchained", ["-DFR_CHECK_UNCHAINED"]), ("planted", ["-DFR_CHECK_PLANT_ERROR"])):
        exe = str(d / ("fr_check_host_" + name))
        subprocess.check_call([cxx, "-O1", "-std=c++17", "-x", "c++", "-DFR_CHECK_HOST", "-Wno-unknown-pragmas"] + defines +
                              ["-I", H.CSRC, H.FR_SOURCE, "-o", exe])
        out[name] = exe
    return out


def run_host(exe, cases):
    return subprocess.run([exe], input=F.encode(cases), capture_output=True, text=True, check=True).stdout


@pytest.mark.parametrize("name", ["product", "unchained"])
def test_every_op_passes_on_the_host_build(host_builds, name):
    """the host test's ops through this harness too (same cases), and the new ones: mul_signed2 with its pairs also
    alone through mul_signed, the first round, the twist, the bit re-slicing, mul_blst"""
    cases, cross = F.all_cases()
    assert {c[0] for c in cases} == set(F.HOST_OPS + F.NEW_OPS)
    per_op = {op: sum(1 for c in cases if c[0] == op) for op in F.NEW_OPS}
    assert all(n >= 100 for n in per_op.values()), per_op
    assert len(cross) == per_op["msig2"]
    bad = F.failures(cases, run_host(host_builds[name], cases), cross)
    assert not bad, "%d cases fail, the first: %s" % (len(bad), bad[:4])


def test_planted_errors_are_found_exactly_on_the_host(host_builds):
    cases, cross = F.all_cases()
    flagged = {(op, i) for op, i, _ in F.failures(cases, run_host(host_builds["planted"], cases), cross)}
    want = {(op, 1) for op in F.HOST_OPS + F.NEW_OPS}
    assert flagged == want, (sorted(flagged - want), sorted(want - flagged))


def test_scan_checker_on_the_models_output_and_a_planted_error():
    """`scan` is device-only; its checker must accept the model's own output and object to one word off by one"""
    cases = F.scan_cases()
    assert sorted({c[1][1][0] for c in cases}) == [1, 2, 4, 8, 16, 32, 64]
    assert len({tuple(c[1][2][:8]) for c in cases}) == len(cases)  # a different C per case
    lines = []
    for _, ops, _ in cases:
        S = [F.wval(ops[0][8 * i:8 * i + 8]) for i in range(64)]
        want = F.scan_model(S, ops[1][0], F.wval(ops[2][:8]))
        # the definition, lane by lane, in plain residues
        gw, C = ops[1][0], F.wval(ops[2][:8]) * F.RINV256 % R
        for lane in (0, 5, 63):
            lg = lane % gw
            plain = sum(pow(C, d, R) * (S[lane + d] * F.RINV256) for d in range(gw - lg)) % R
            assert want[lane] * F.RINV256 % R == plain
        lines.append(" ".join("%x" % w for v in want for w in F.words(v)))
    assert F.failures(cases, "\n".join(lines)) == []
    words = lines[1].split()
    words[8 * 37 + 3] = "%x" % ((int(words[8 * 37 + 3], 16) + 1) & 0xFFFFFFFF)
    lines[1] = " ".join(words)
    assert [(op, i) for op, i, _ in F.failures(cases, "\n".join(lines))] == [("scan", 1)]


# ------------------------------------------------------------------------------------------------ the model
SHAPES = [("fwd", 12), ("inv", 12), ("fwd", 9), ("inv", 9), ("fwd", 6), ("fwd", 13), ("fwd", 14), ("inv", 14), ("das", 12), ("das", 8)]


@pytest.fixture(scope="module")
def vectors():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert int(doc["r"], 16) == R
    return doc["vectors"]


@pytest.fixture(scope="module")
def runs(vectors):
    """every stored vector through the model, once: name -> (reached per target, largest value, outputs)"""
    return {v["name"]: M.run_vector(v) for v in vectors}


@pytest.fixture(scope="module")
def random_tops():
    """(shape, logn) -> per pass, the largest value that reaches reduce_lazy / finish over three random vectors"""
    return {(shape, L): M.random_top(L, shape) for shape, L in SHAPES}


@pytest.mark.parametrize("shape,L", SHAPES)
def test_model_residues_equal_a_plain_transform(shape, L):
    """the model's outputs against the textbook recursive transform (all outputs) and against the definition
    sum x_k w^(jk) (a few outputs), on a random vector with 0, r - 1 and 2^256 - 1 in it"""
    rnd = random.Random(40 + L)
    n = 1 << L
    x = [rnd.randrange(R) for _ in range(n)]
    x[0], x[n // 2], x[n - 1] = R - 1, 0, (1 << 256) - 1
    if shape == "das":
        res = M.das(x, L)
        assert res["out"] == M.das_reference(x, L)
        c = M.dft_fast(x, L, inverse=True)
        w2 = pow(7, (R - 1) >> (L + 1), R)
        c = [v * pow(w2, j, R) % R for j, v in enumerate(c)]
        outs = [0, 1, n // 3, n - 1]
        assert M.dft_direct(x, L, outs, inverse=True) == {j: M.dft_fast(x, L, inverse=True)[j] for j in outs}
        assert M.dft_direct(c, L, outs) == {j: res["out"][j] for j in outs}
    else:
        res = M.transform(x, L, shape == "inv")
        assert res["out"] == M.dft_fast(x, L, shape == "inv")
        outs = [0, 1, n // 3, n - 2, n - 1]
        assert M.dft_direct(x, L, outs, shape == "inv") == {j: res["out"][j] for j in outs}
    assert res["top"] < 64 * R


def test_the_stored_vectors_are_the_ones_the_issue_lists(vectors):
    by = {v["name"]: v for v in vectors}
    assert len(by) == len(vectors)
    assert {(v["shape"], v["logn"]) for v in vectors} == set(SHAPES)
    for shape in ("fwd", "inv"):
        assert by[shape + "4096_last"]["targets"] == [[0, 0, 4095]] and by[shape + "4096_bf1n"]["targets"] == [[0, 0, 4094]]
    for name, L in (("fwd512_tile", 9), ("fwd64_tile", 6)):
        v = by[name]
        assert v["nbatch"] << L == 4096  # the batch fills a tile
        t = [o for _, _, o in v["targets"]]
        assert all(a != b for a, b in zip(t, t[1:])) and len(t) == v["nbatch"]
    for L in (13, 14):
        assert by["fwd2p%d_first_pass" % L]["targets"][0][1] == 0 and by["fwd2p%d_second_pass" % L]["targets"][0][1] == 1
    assert by["das4096"]["space"] == by["das256"]["space"] == "fwd_half"
    assert int(by["fwd4096_fill_r_minus_1"]["fill"], 16) == R - 1
    nc = by["fwd4096_fill_2p256_minus_1"]
    assert int(nc["fill"], 16) == int(nc["x0"][0], 16) == (1 << 256) - 1
    for v in vectors:  # sparse: a chain's start and one input per stage
        assert len(v["entries"]) <= v["nbatch"] * (v["logn"] + 2)


def test_every_stored_vector_reaches_its_recorded_value(vectors, runs):
    for v in vectors:
        reached, top, outs = runs[v["name"]]
        assert ["%x" % r for r in reached] == v["reached"], v["name"]
        assert top < 64 * R, "%s: a value of %.2fr" % (v["name"], top / R)  # nothing anywhere in the run reaches 64r
        rows = M.materialise(v)
        for row, out in zip(rows[:2], outs[:2]):  # and the model's residues are the transform's
            want = M.das_reference(row, v["logn"]) if v["shape"] == "das" else M.dft_fast(row, v["logn"], v["shape"] == "inv")
            assert out == want, v["name"]


def bound_of(v, k):
    b, p, o = v["targets"][k]
    Ts = M.split_passes(v["logn"])
    x0 = int(v["x0"][k], 16)
    if p == 0 or v["shape"] == "das":
        return M.path_bound(x0, o, 0, Ts[0], True)
    return M.path_bound(x0, o, Ts[0], Ts[1], False)


def test_path_bound_is_the_issues_formula():
    for T in (6, 7, 8, 9, 12):
        assert M.path_bound(R - 1, (1 << T) - 1, 0, T, True) == R - 1 + 4 * R + 5 * R * (T - 1)
        assert M.path_bound(2 * R - 1, (1 << T) - 1, 0, T, True) == 2 * R - 1 + 4 * R + 5 * R * (T - 1)
    assert M.path_bound(R, (1 << 14) - 1, 7, 7, False) == R + 5 * R * 7
    # the x + 8r - y branch: x = x0 + y0 < 2r after stage 0, so the same 10r after two stages
    assert M.path_bound(R - 1, 4094, 0, 12, True) == (R - 1) + R + 8 * R + 50 * R


def test_aimed_vectors_reach_where_random_inputs_do_not(vectors, runs, random_tops):
    by = {v["name"]: v for v in vectors}
    first = int(by["fwd4096_last"]["reached"][0], 16)
    assert first >= 57 * R, "%.3fr" % (first / R)
    for v in vectors:
        reached = runs[v["name"]][0]
        for k, (b, p, o) in enumerate(v["targets"]):
            bound = bound_of(v, k)
            rnd_top = random_tops[(v["shape"], v["logn"])][p]
            what = "%s[%d]: reached %.3fr, path bound %.3fr, random %.3fr" % (v["name"], k, reached[k] / R, bound / R, rnd_top / R)
            assert bound - 4 * R < reached[k] < bound, what
            if bound - 3 * R > rnd_top:
                assert reached[k] >= rnd_top + 3 * R, what
            else:  # no input can be 3r above random here (module docstring)
                assert M.split_passes(v["logn"])[p] <= 7, what
                assert reached[k] > bound - R and reached[k] > rnd_top, what


def test_the_quotients_random_vectors_miss_are_covered(vectors, runs, random_tops):
    """reduce_lazy's quotient floor(value / r) for the forward 4096-point vectors: random inputs stop at 53, the stored
    ones reach 57 and 58"""
    assert random_tops[("fwd", 12)][0] // R <= 53
    got = {runs[name][0][0] // R for name in ("fwd4096_last", "fwd4096_bf1n", "fwd4096_fill_r_minus_1", "fwd4096_fill_2p256_minus_1")}
    assert got >= {57, 58}, got
    assert runs["das4096"][0][0] // R >= 57 and runs["inv4096_bf1n"][0][0] // R >= 58


def test_model_pass_structure_is_the_planners():
    """split_passes and the unit stages against tools/ntt_plan_sim.py, the prototype the C++ planner is ported from: a
    first pass of T >= 2 stages opens with a two-stage round at position 0 (stages 0 and 1 are the unit stages), the
    fused DAS plan marks exactly the first round of each half as unit and the last inverse round as the twist"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("ntt_plan_sim", os.path.join(H.ROOT, "tools", "ntt_plan_sim.py"))
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    for L in range(13, 31):
        assert M.split_passes(L) == sim.split_passes(L)
    assert all(M.split_passes(L) == [L] for L in range(0, 13)) and sim.LOGT == M.LOGT == 12
    for kind, Ts in ((sim.KIND_A1, range(2, 13)), (sim.KIND_A2, range(2, 11))):
        for T in Ts:
            ph = sim.phases_for(kind, T)
            assert sim.rounds_of_phase(ph[0][0], ph[0][1])[0] == (0, 2)
    for T in (8, 12):
        rounds = sim.plan_das(T)["rounds"]
        assert [r for r, Rd in enumerate(rounds) if Rd["unit"]] == [0, len(rounds) // 2]
        assert [r for r, Rd in enumerate(rounds) if Rd["twist"]] == [len(rounds) // 2 - 1]
        assert [Rd["part"] for Rd in rounds] == [0] * (len(rounds) // 2) + [1] * (len(rounds) // 2)
