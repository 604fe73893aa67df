"""What the GPU tests of the Fp2 / G2 lane arithmetic (tests/test_g2_arith_gpu.py) rest on, checked without a GPU:

  * tests/device_checks/g2_check.hip cross-compiles for gfx950 in every define set, with the product's flags;
  * the case lists of tests/g2_lane_cases.py build with every precondition holding (the generators assert them), hold
    the per-op minimum, the wave mixes, and the edges the headers' tables name — looked for here as literal values;
  * every op passes on the harness's host form (-DG2_CHECK_HOST), with and without the filter of the exact zero test,
    and the planted errors of -DG2_CHECK_PLANT_ERROR are found exactly;
  * every checker rejects a result that is one limb off, a wrong point, and a wrong verdict;
  * the model's G2 arithmetic agrees with host_pairing.h on a handful of points, through the stand-alone host program
    of tests/test_g2_lane_cpu.py (nothing preloaded, no sanitizer).

The module prints the seconds it spends on the cases, the host runs and the cross-compilation."""
import os
import random
import subprocess
import time

import pytest

import codec_model as CM
import g2_encodings as G2E
import g2_lane_cases as G
import lane_harness as H
import setup_model as S
import test_g2_lane_cpu as L

P = G.P
VERDICT_OPS = {"fp_iszero": 0, "f2_iszero": 0, "io_lex": 0, "io_sqrt": 0, "io_uncompress": 0, "io_ing2": 0}
# the word of an op's output that the limb-off probe spoils (a limb of the first component, or a byte)
PROBE_WORD = {"g2_madd": 1 + 5, "io_sqrt": 1 + 5, "io_uncompress": 2 + 5, "io_compress": 50, "io_psiconst": 14 + 5}


# ------------------------------------------------------------------------------------------------ the harness
@pytest.fixture(scope="module")
def cross_compiled(tmp_path_factory):
    if not os.path.exists(H.product_build().hipcc_path()):
        pytest.skip("no hipcc on this machine")
    sets = dict(H.G2_DEFINE_SETS)
    sets.update(H.G2_PLANTED)
    began = time.time()
    res = H.compile_all(tmp_path_factory.mktemp("g2_check"), sets, H.G2_SOURCE)
    print("g2_check.hip: %d device builds side by side in %.0f s" % (len(sets), time.time() - began))
    return res


@pytest.mark.parametrize("name", list(H.G2_DEFINE_SETS) + list(H.G2_PLANTED))
def test_g2_harness_cross_compiles_for_gfx950(cross_compiled, name):
    """a header change that breaks tests/device_checks/g2_check.hip shows here, on a machine without a GPU"""
    built, errors = cross_compiled
    assert name in built, errors.get(name)
    defines = H.G2_DEFINE_SETS.get(name, H.G2_PLANTED.get(name))
    cmd = H.compile_command("x", defines, H.G2_SOURCE)
    b = H.product_build()
    assert cmd[0] == b.hipcc_path() and cmd[1:1 + len(b.COMPILE_FLAGS)] == list(b.COMPILE_FLAGS)
    assert "--offload-arch=gfx950" in cmd and "-O3" in cmd and "-std=c++17" in cmd and H.G2_SOURCE in cmd
    assert H.G2_DEFINE_SETS == {"product": [], "exact": ["-DKZGAMD_FORCE_EXACT_TESTS"]}


@pytest.fixture(scope="module")
def blocks():
    began = time.time()
    b = G.all_cases()
    print("g2_lane_cases.all_cases(): %d cases in %.1f s" % (sum(len(v) for v in b.values()), time.time() - began))
    return b


@pytest.fixture(scope="module")
def host_builds(tmp_path_factory):
    """g2_check.hip's host form: the same op bodies over the same headers, no HIP; compiled side by side"""
    d = tmp_path_factory.mktemp("g2_check_host")
    procs = {}
    for name, defines in (("product", []), ("exact", ["-DKZGAMD_FORCE_EXACT_TESTS"]), ("planted", ["-DG2_CHECK_PLANT_ERROR"])):
        exe = str(d / ("g2_check_host_" + name))
        procs[name] = (exe, subprocess.Popen(H.host_compile_command(exe, defines)))
    for name, (exe, p) in procs.items():
        assert p.wait() == 0, name
    return {name: exe for name, (exe, _) in procs.items()}


@pytest.fixture(scope="module")
def host_outputs(host_builds, blocks):
    """name -> block -> outputs of every case, one run per build"""
    text = G.encode(blocks)
    outs = {}
    for name, exe in host_builds.items():
        began = time.time()
        run = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert run.returncode == 0, (name, run.stdout[-300:], run.stderr[-300:])
        outs[name] = G.decode(run.stdout, blocks)  # as many lines as cases, every line as long as the op's output
        print("host form, %s: %.1f s" % (name, time.time() - began))
    return outs


# ------------------------------------------------------------------------------------------------ the cases
def test_case_lists_hold_their_minimum_and_their_waves(blocks):
    per_op = G.cases_per_op(blocks)
    assert set(per_op) == set(G.OPS) and all(n >= 64 for n in per_op.values())
    assert all(per_op[op] >= 128 for op in G.POINT_OPS + ("lc_term",))
    assert {b for layer in G.LAYERS.values() for b in layer} == set(blocks)
    for op in G.POINT_OPS + ("lc_term",):
        mixed, uni = blocks[op + "/mixed"], blocks[op + "/uniform"]
        kinds = {c.kind for c in mixed}
        assert "generic" in kinds and len(kinds) >= 4, (op, kinds)
        for w in range(0, len(mixed), 64):  # every wave, the partial last one too, holds every kind
            assert {c.kind for c in mixed[w:w + 64]} == kinds, (op, w)
        assert len(uni) % 64 == 0
        for w in range(0, len(uni), 64):
            assert len({c.kind for c in uni[w:w + 64]}) == 1, (op, w)
    assert any(len(blocks[op + "/mixed"]) % 64 for op in G.POINT_OPS)
    uk = lambda op: {c.kind for c in blocks[op + "/uniform"]}
    assert {"P + P", "P - P", "infinity + P"} <= uk("g2_madd") and uk("g2_madd") == uk("g2_maddc")
    assert {"flagged", "P + P", "P - P"} <= uk("g2_maddtab") and {"P + P", "P - P", "infinity + Q"} <= uk("g2_add")
    assert {"zero scalar", "identity"} <= uk("lc_term")
    assert set(G.MADD_KINDS) == {c.kind for c in blocks["g2_madd/mixed"]} and set(G.TAB_KINDS) == {c.kind for c in blocks["g2_maddtab/mixed"]}
    assert set(G.ADD_KINDS) == {c.kind for c in blocks["g2_add/mixed"]}
    for w in range(0, len(blocks["lc_term/mixed"]), 64):
        assert {"short", "long", "zero scalar", "identity", "order 13"} <= {c.kind for c in blocks["lc_term/mixed"][w:w + 64]}


def test_the_edges_the_tables_name_are_there_as_literal_values(blocks):
    nl, M28 = G.nl, G.M28
    fe = lambda c, k: tuple(c.words[14 * k:14 * k + 14])
    has = lambda block, k, limbs: any(fe(c, k) == tuple(limbs) for c in blocks[block])
    # products: 30-bit limbs on both sides, the largest values, k p and its neighbours, an empty top limb
    lazy7 = [(1 << 30) - 1] * 7 + [0] * 7
    assert any(fe(c, 0) == tuple(lazy7) == fe(c, 1) for c in blocks["fp_mul"]) and has("fp_sqr", 0, lazy7)
    assert has("fp_mul", 0, [(1 << 30) - 1] * 13 + [0]) and has("fp_mul", 0, nl(63 * P - 1)) and has("fp_mul", 1, nl(40 * P - 1))
    assert all(has("fp_mul", 0, nl(P + d)) for d in (-1, 0, 1)) and has("fp_mul", 0, nl((1 << 364) - 1))
    assert has("fp_sqr", 0, nl(50 * P - 1)) and has("fp_sqr", 0, nl(0))
    mx = [G.LAZY_LIMB - 1] * 13
    assert any(fe(c, 1)[:13] == tuple(mx) == fe(c, 3)[:13] for c in blocks["fp_mul2"])  # the columns at their bound
    # subtractions: b at the top of what the pad admits, on every pad
    for k in (2, 4, 8, 16, 32):
        for op in ("fp_sub%d", "fp_subl%d"):
            assert has(op % k, 1, nl((k - 1) * P - 1)) and has(op % k, 1, nl(0)) and has(op % k, 1, nl((k - 2) * P))
        assert has("fp_neg%d" % k, 0, nl((k - 1) * P - 1)) and has("fp_neg%d" % k, 0, nl(0))
        assert any(fe(c, 1)[:13] == (M28,) * 13 for c in blocks["fp_sub%d" % k])  # limbs 0..12 all ones
    for m in (0, 0xFFFFFFFF):  # s and y at their maxima, both masks
        assert any(fe(c, 0) == tuple(nl(2 * P - 1)) and fe(c, 1) == tuple(nl(6 * P - 1)) and c.words[28] == m for c in blocks["fp_ssl16"])
        assert any(fe(c, 0) == tuple(nl(P - 1)) and fe(c, 1) == tuple(nl(2 * P)) and c.words[28] == m for c in blocks["fp_ssl8"])
    assert any(fe(c, 1) == tuple(nl(2 * P - 1)) == fe(c, 2) for c in blocks["fp_sub2bc"])
    # the exact zero test: every multiple, its neighbours, at least 64 of the filter's false positives
    for j in range(64):
        assert has("fp_iszero", 0, nl(j * P))
        assert has("fp_iszero", 0, nl(j * P + 1)) or j == 63 and has("fp_iszero", 0, nl(j * P + 1))
    assert sum(1 for j in range(63) if has("fp_iszero", 0, nl(j * P + (1 << 200))) and has("fp_iszero", 0, nl(j * P + (1 << 364)))) == 63
    passes = [c for c in blocks["fp_iszero"] if (c.words[0] & M28) * 0x0030003 & M28 < 64 and G.value(c.words) % P and G.normalized(c.words)]
    assert len(passes) >= 64
    assert sum(1 for c in blocks["fp_iszero"] if any(x > M28 for x in c.words[:13])) >= 16  # lazy sums
    # Fp2: a residue plus (K - 1) p on every component of both operands, for every row of the table
    for name, ba, bb, _ in G.F2_TABLE:
        cs = blocks["f2_" + name]
        assert any(all(G.value(fe(c, k)) >= (ba - 1) * P for k in (0, 1)) for c in cs), name
        if name not in G.F2_UNARY and name != "mulfe":
            assert any(all(G.value(fe(c, k)) >= (bb - 1) * P for k in (2, 3)) for c in cs), name
        assert any(fe(c, 0)[:13] == (M28,) * 13 for c in cs) and any(fe(c, 0)[:13] == (0,) * 13 and fe(c, 0)[13] > 0 for c in cs) or ba == 1, name
    # points: X, Y at 14 p and Z at 20 p into dbl; X, Y at 2 p and Z at 9 p into the additions
    at_top = lambda c, tops, base=0: all(G.value(fe(c, base + k)) >= t * P for k, t in enumerate(tops))
    assert sum(1 for c in blocks["g2_dbl/mixed"] if at_top(c, G.TOP_DBL)) >= 30 and all(at_top(c, G.TOP_DBL) for c in blocks["g2_dbl/uniform"])
    for b in ("g2_madd/mixed", "g2_maddc/mixed", "g2_maddtab/mixed", "g2_add/mixed", "g2_madd/uniform", "g2_add/uniform"):
        assert sum(1 for c in blocks[b] if at_top(c, G.TOP_MADD)) >= 30, b
    assert sum(1 for c in blocks["g2_add/mixed"] if at_top(c, G.TOP_MADD) and at_top(c, G.TOP_MADD, 6)) >= 30
    assert any(c.words[140] == 1 and c.words[141] == 0xFFFFFFFF for c in blocks["g2_maddtab/mixed"])  # flagged, both signs
    assert any(c.words[140] == 1 and c.words[141] == 0 for c in blocks["g2_maddtab/mixed"])
    assert any(c.words[:84] == [0] * 84 and c.words[140] == 0 for c in blocks["g2_maddtab/mixed"])  # onto infinity
    assert any(at_top(c, G.TOP_AFF) for c in blocks["g2_toaff"]) and any(c.words[56:84] == [0] * 28 for c in blocks["g2_toaff"])
    # g2io
    for v in (0, P - 1, P, P + 1, 2 * P - 1, 2 * P):
        assert has("io_canon2", 0, nl(v))
    half = (P - 1) // 2
    for c0 in (0, 1, half, half + 1, P - 1):
        assert any(fe(c, 0) == tuple(nl(G.rep(c0, 0))) and G.value(fe(c, 1)) % P == 0 for c in blocks["io_lex"]), c0
    for c1 in (1, half, half + 1, P - 1):
        assert any(fe(c, 1) == tuple(nl(G.rep(c1, 1))) for c in blocks["io_lex"]), c1
    assert len(G.LEX_VALUES) == 9
    tags = {c.tag.split(" + ")[0] for c in blocks["io_sqrt"]}
    assert tags == {"zero", "square", "non-square", "purely real, a residue", "purely real, t == 0: a1 = 0 and s = -a0", "purely imaginary"}
    for t in tags:  # each also with 63 p on top of both components
        assert any(c.tag == t + " + (63, 63) p" and all(G.value(fe(c, k)) >= 63 * P for k in (0, 1)) for c in blocks["io_sqrt"]), t
    cat = G2E.catalogue()
    assert [bytes(c.words) for c in blocks["io_uncompress"]] == [b for _, b, _ in cat]
    valid = [name for name, _, cls in cat if cls != 1]
    assert [c.tag for c in blocks["io_ing2"]][:len(valid)] == valid == [c.tag for c in blocks["io_compress"]][:len(valid)]
    # g2lc::term: every scalar case, in Montgomery form, over one generator multiple with Z != 1
    base = [c for c in blocks["lc_term/mixed"] if c.kind in ("generic", "short", "long", "zero scalar")]
    sent = {tuple(c.words[72:]) for c in base}
    assert all(tuple(G.w32(k * (1 << 256) % S.R, 8)) in sent for k in S.scalar_cases())
    one = G.w32((1 << 384) % P, 12)
    assert all(c.words[48:60] != one for c in base)  # Z != 1
    thin = G.thinned_scalars()
    fam = S.family_2k()
    assert all(k in thin for k in S.scalar_cases() if k not in fam) and all(fam[k] % 8 == 0 for k in thin if k in fam)
    assert sum(1 for c in blocks["lc_term/mixed"] if c.kind == "order 13") == len(thin) == sum(1 for c in blocks["lc_term/mixed"] if c.kind == "identity")


def test_the_models_term_is_the_plain_double_and_add():
    """FixedBase (windows, Jacobian sums, one inversion) against codec_model.mul, the textbook affine walk"""
    rnd = random.Random(5)
    a = CM.mul(7, CM.G2)
    began = time.time()
    fb = G.FixedBase(a)
    for k in [0, 1, 2, 255, 256, S.R - 1, (1 << 254) - 1] + [rnd.randrange(S.R) for _ in range(4)]:
        assert fb.mul(k) == CM.mul(k, a)
    t = CM.torsion_point(13)
    ft = G.FixedBase(t)  # tables with infinite entries, sums that meet: the exceptional branches of the model
    for k in (13, 26, 14, 12, 1 << 200, S.R - 1):
        assert ft.mul(k) == CM.mul(k % 13, t)
    print("model of term: two tables and %d products in %.1f s" % (17, time.time() - began))


# ------------------------------------------------------------------------------------------------ the host form
@pytest.mark.parametrize("name", ["product", "exact"])
def test_every_op_passes_on_the_host_build(host_outputs, blocks, name):
    bad = G.failures(blocks, host_outputs[name])
    assert not bad, "%d cases fail, the first: %s" % (len(bad), bad[:4])


def test_planted_errors_are_found_exactly_on_the_host(host_outputs, blocks):
    flagged = {(b, i) for b, i, _ in G.failures(blocks, host_outputs["planted"])}
    want = {(b, 1) for b in blocks}
    assert flagged == want, (sorted(flagged - want), sorted(want - flagged))


def rejects(case, out):
    try:
        case.check(out)
    except AssertionError:
        return True
    return False


def test_every_checker_rejects_one_limb_off_a_wrong_point_and_a_wrong_verdict(host_outputs, blocks):
    good = host_outputs["product"]
    for block, cases in blocks.items():
        op = G.op_of(block)
        for i in (0, 2, len(cases) - 1):
            out = list(good[block][i])
            assert not rejects(cases[i], out)
            if op in VERDICT_OPS:  # a wrong verdict
                out[VERDICT_OPS[op]] ^= 1
                assert rejects(cases[i], out), (block, i, "verdict")
                out = list(good[block][i])
            if len(out) > 1:  # one limb (or byte) off, up and down
                w = PROBE_WORD.get(op, 5)
                for d in (1, -1):
                    spoiled = list(out)
                    spoiled[w] = (spoiled[w] + d) & 0xFFFFFFFF
                    if op in ("io_sqrt", "io_uncompress") and out[0] == 0:
                        continue  # no root / no point to spoil
                    assert rejects(cases[i], spoiled), (block, i, "limb %+d" % d)
    # a wrong point: the answer of another case of the block, itself a correct, normalized point
    for block in [op + "/mixed" for op in G.POINT_OPS + ("lc_term",)] + ["g2_fedback", "lc_tree1", "lc_tree6", "g2_toaff", "io_psi"]:
        cases, outs = blocks[block], good[block]
        swapped = 0
        for i in range(len(cases) - 1):
            other = outs[i] != outs[i + 1]
            if len(outs[i]) in (84, 85):  # another representation of the same point is no wrong point
                pt = lambda o: (o[:-84], G.affine_of([o[len(o) - 84 + 14 * k:len(o) - 70 + 14 * k] for k in range(6)]))
                other = pt(outs[i]) != pt(outs[i + 1])
            if other and any(outs[i + 1][-28:]) and any(outs[i][-28:]):
                assert rejects(cases[i], outs[i + 1]), (block, i)
                swapped += 1
        assert swapped >= 16, block
    # -P for P: a point on the curve with the right x
    for block in ("g2_add/mixed", "g2_dbl/mixed", "lc_term/mixed"):
        done = 0
        for c, o in zip(blocks[block], good[block]):
            if any(o[56:]) and c.kind == "generic":
                y = [G.nl(2 * P - G.value(o[28 + 14 * k:42 + 14 * k])) for k in (0, 1)]
                if all(G.value(v) < 2 * P for v in y):
                    assert rejects(c, o[:28] + y[0] + y[1] + o[56:]), block
                    done += 1
        assert done >= 8, block


def test_the_model_agrees_with_the_host_specification(tmp_path):
    """the chord / tangent law and FixedBase against host_pairing.h's g2_dbl / g2_add, through the stand-alone program of
    tests/test_g2_lane_cpu.py: the program compares g2_28.hip.h with host_pairing.h (its last column), the model's point
    is compared here with what it printed"""
    rnd = random.Random(0x77)
    cmd, exe = L.compile_program(tmp_path, "g2model", [])
    subprocess.check_call(cmd)
    s = L.Script()
    wants = []
    base = CM.mul(5, CM.G2)
    fb = G.FixedBase(base)
    for k in (1, 2, 3, 1000, S.R - 2):
        a = fb.mul(k)
        s.dbl(s.jac(a, (rnd.randrange(P), rnd.randrange(P)), [0] * 6), None)
        wants.append(fb.mul(2 * k % S.R))
        s.madd(s.jac(a, (rnd.randrange(P), rnd.randrange(P)), [0] * 6), [G.rep(c, 0) for c in base[0] + base[1]], L.DONE, None, "model")
        wants.append(fb.mul((k + 1) % S.R))
    run = subprocess.run([str(exe)], input="\n".join(s.lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-1000:]
    out = run.stdout.strip().split("\n")
    assert len(out) == len(wants) == 10
    for (tag, _, _), ln, want in zip(s.checks, out, wants):
        t = [int(x, 16) for x in ln.split()]
        assert t[-1] == 1, "g2_28.hip.h differs from host_pairing.h"
        body = t[1:-1] if tag[0] == "M" else t[:-1]
        assert G.affine_of([body[14 * k:14 * k + 14] for k in range(6)]) == want, tag
