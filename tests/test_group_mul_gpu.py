"""kzgamd_g1_mul_batch / kzgamd_g2_mul_batch (groupmul.hip: a window table of the base, one lane per output) through
the C ABI, on both library flavours.  Anchors, neither of them the code under test: the CPU oracle's og1_mul for G1, the
host's kzgamd_p2_mult (host_pairing.h, compared through kzgamd_p2_compress) for G2.  The scalar list is
tests/setup_model.py's, which does not know the window width.

G2 scalars: the host reference for the whole list (872 scalars) takes 0.2 s on one CPU core, far under the 5 s that
would have thinned it, so the whole list runs in G2 too: kept count = 872, all of them."""
import ctypes as C
import random

import pytest

import g1_encodings as E
import oracle_ffi as O
import setup_model as S

pytestmark = pytest.mark.gpu
R = S.R
CASES = S.scalar_cases()
_ref = {}


def fr_bulk(kzg, vals):
    raw = b"".join(((v << 256) % R).to_bytes(32, "little") for v in vals)
    arr = (kzg.BlstFr * max(len(vals), 1))()
    C.memmove(arr, raw, len(raw))
    return arr


def og1(p):
    g = O.G1()
    C.memmove(C.byref(g), bytes(p), 144)
    return g


def to_p1(kzg, g):
    p = kzg.BlstP1()
    C.memmove(C.byref(p), bytes(g), 144)
    return p


def g1_base(name):
    """the oracle's generator, [7]G, and 2 * [7]G with whatever Z og1_dbl leaves (not normalised)"""
    if ("g1base", name) not in _ref:
        L = O.lib()
        g = O.G1()
        L.og1_generator(C.byref(g))
        if name != "gen":
            seven = O.G1()
            L.og1_mul(C.byref(seven), C.byref(g), C.byref(O.fr_from_int(7)))
            g = seven
            if name == "dbl":
                d = O.G1()
                L.og1_dbl(C.byref(d), C.byref(seven))
                assert bytes(d)[96:144] != bytes(seven)[96:144]  # another Z
                g = d
        _ref[("g1base", name)] = g
    return _ref[("g1base", name)]


def g1_expected(name, vals):
    """[v] base from the oracle (None for the identity), computed once per (base, scalar)"""
    L = O.lib()
    base = g1_base(name)
    out = []
    for v in vals:
        key = ("g1", name, v)
        if key not in _ref:
            if v == 0:
                _ref[key] = None
            else:
                e = O.G1()
                L.og1_mul(C.byref(e), C.byref(base), C.byref(O.fr_from_int(v)))
                _ref[key] = e
        out.append(_ref[key])
    return out


def assert_g1(got, exp, what):
    L = O.lib()
    for j, e in enumerate(exp):
        g = og1(got[j])
        if e is None:
            assert L.og1_is_inf(C.byref(g)) and bytes(got[j]) == bytes(144), (what, j, "expected the identity, all-zero")
        else:
            assert not L.og1_is_inf(C.byref(g)) and L.og1_equal(C.byref(g), C.byref(e)), (what, j)


def g2_base(kzg, name):
    if ("g2base", name) not in _ref:
        g = kzg.p2_generator()
        if name != "gen":
            seven = kzg.p2_mult(g, fr_bulk(kzg, [7])[0])
            g = seven
            if name == "add":
                g = kzg.p2_add(seven, kzg.p2_mult(kzg.p2_generator(), fr_bulk(kzg, [5])[0]))  # [12]G2, Z not one
                assert bytes(g)[192:288] != bytes(kzg.p2_generator())[192:288]
        _ref[("g2base", name)] = bytes(g)
    p = kzg.BlstP2()
    C.memmove(C.byref(p), _ref[("g2base", name)], 288)
    return p


def g2_expected(kzg, name, vals):
    """compressed [v] base by the host's double-and-add, once per (base, scalar)"""
    base = g2_base(kzg, name)
    frs = fr_bulk(kzg, vals)
    out = []
    for i, v in enumerate(vals):
        key = ("g2", name, v)
        if key not in _ref:
            _ref[key] = kzg.p2_compress(kzg.p2_mult(base, frs[i]))
        out.append(_ref[key])
    return out


INF2 = bytes([0xc0]) + bytes(95)


def assert_g2(kzg, got, exp, what):
    for j, e in enumerate(exp):
        assert kzg.p2_compress(got[j]) == e, (what, j)
        if e == INF2:
            assert bytes(got[j]) == bytes(288), (what, j, "the identity is all-zero")


def subset():
    rnd = random.Random(7)
    return CASES[:6] + CASES[6::16] + rnd.sample(CASES, 24)


def test_g1_every_scalar_case_against_the_oracle(kzg):
    assert len(CASES) > 800 and CASES[0] == 0
    got = kzg.g1_mul_batch(fr_bulk(kzg, CASES), len(CASES))
    assert_g1(got, g1_expected("gen", CASES), "generator (base = NULL)")


def test_g2_every_scalar_case_against_the_host_multiplication(kzg):
    got = kzg.g2_mul_batch(fr_bulk(kzg, CASES), len(CASES))
    exp = g2_expected(kzg, "gen", CASES)
    assert exp[0] == INF2 and exp[1] == kzg.p2_compress(kzg.p2_generator())
    assert_g2(kzg, got, exp, "generator (base = NULL)")


def test_bases_explicit_generator_a_multiple_and_a_z_that_is_not_one(kzg):
    vals = subset()
    sc = fr_bulk(kzg, vals)
    for name in ("gen", "seven", "dbl"):
        got = kzg.g1_mul_batch(sc, len(vals), base=to_p1(kzg, g1_base(name)))
        assert_g1(got, g1_expected(name, vals), "G1 base " + name)
    for name in ("gen", "seven", "add"):
        got = kzg.g2_mul_batch(sc, len(vals), base=g2_base(kzg, name))
        assert_g2(kzg, got, g2_expected(kzg, name, vals), "G2 base " + name)


def test_a_base_at_infinity_and_a_g1_base_outside_the_subgroup(kzg):
    L = kzg.lib()
    sc = fr_bulk(kzg, CASES[:5])
    out1, out2 = (kzg.BlstP1 * 5)(), (kzg.BlstP2 * 5)()
    C.memset(out1, 0x5a, C.sizeof(out1))
    C.memset(out2, 0x5a, C.sizeof(out2))
    assert L.kzgamd_g1_mul_batch(out1, C.byref(kzg.BlstP1()), sc, 5, None) == 0 and bytes(out1) == bytes(5 * 144)
    assert L.kzgamd_g2_mul_batch(out2, C.byref(kzg.BlstP2()), sc, 5, None) == 0 and bytes(out2) == bytes(5 * 288)
    # a point of order 11 of the curve: on it, not in the subgroup
    x, y = E.torsion_point(11)
    low = kzg.BlstP1()
    C.memmove(C.byref(low), b"".join(((v << 384) % E.P).to_bytes(48, "little") for v in (x, y, 1)), 144)
    C.memset(out1, 0x5a, C.sizeof(out1))
    assert L.kzgamd_g1_mul_batch(out1, C.byref(low), sc, 5, None) == 3 and bytes(out1) == b"\x5a" * (5 * 144)


def twist_bases():
    """two points of E'(Fp2) outside the subgroup, as affine Python integers: one of order 13 (13^2 divides the cofactor)
    and a random one of full order; cached"""
    if "twist" not in _ref:
        from test_g2_lane_cpu import aff_add, twist_point

        def mul(k, a):
            r = None
            while k:
                if k & 1:
                    r = aff_add(r, a)
                a = aff_add(a, a)
                k >>= 1
            return r

        x = -0xd201000000010000
        h2 = (x**8 - 4 * x**7 + 5 * x**6 - 4 * x**4 + 6 * x**3 - 4 * x**2 - 4 * x + 13) // 9  # #E'(Fp2) = h2 * r
        assert h2 % 169 == 0 and h2 % 2 == 1
        rnd = random.Random(13)
        while True:
            q = twist_point(rnd)
            assert mul(h2 * R, q) is None
            t = mul(h2 * R // 169, q)
            if t is None:
                continue
            if mul(13, t) is not None:
                t = mul(13, t)
            assert mul(13, t) is None
            assert mul(R, q) is not None  # q itself: not in the subgroup
            _ref["twist"] = {"order13": t, "full": q}
            break
    return _ref["twist"]


def p2_from_affine(kzg, a):
    (x0, x1), (y0, y1) = a
    p = kzg.BlstP2()
    raw = b"".join(((v << 384) % E.P).to_bytes(48, "little") for v in (x0, x1, y0, y1, 1, 0))
    C.memmove(C.byref(p), raw, 288)
    return p


@pytest.mark.parametrize("which", ["order13", "full"])
def test_g2_base_outside_the_subgroup_is_still_the_group_law(kzg, which):
    """The header's promise for a G2 base it does not test.  A base of order 13 has a table whose entries 13, 26, ... of
    every window are infinity, and its walk meets P + P and P - P all the time: the flag, MADD_DOUBLE and MADD_INF
    all run.  Against kzgamd_p2_mult (complete double-and-add on the host) through kzgamd_p2_compress."""
    base = p2_from_affine(kzg, twist_bases()[which])
    rnd = random.Random(26)
    vals = CASES[:6] + list(range(3, 40)) + [13 * 256 ** k for k in (1, 7, 31) if 13 * 256 ** k < R] + CASES[6::9] + rnd.sample(CASES, 40)
    sc = fr_bulk(kzg, vals)
    got = kzg.g2_mul_batch(sc, len(vals), base=base)
    want = [kzg.p2_compress(kzg.p2_mult(base, sc[i])) for i in range(len(vals))]
    ninf = 0
    for j in range(len(vals)):
        assert kzg.p2_compress(got[j]) == want[j], (which, j, hex(vals[j]))
        if want[j] == INF2:
            assert bytes(got[j]) == bytes(288), (which, j)
            ninf += 1
    if which == "order13":
        assert ninf >= 5 and any(w != INF2 for w in want)  # multiples of 13 among the scalars, and others
    else:
        assert ninf == 1  # the scalar 0 alone


@pytest.mark.parametrize("tuning,counts", [(None, (0, 1, 63, 64, 65, 255, 256, 257)), ("mul_slice=64", (64, 65, 129))])
def test_counts_and_slice_edges(kzg, tuning, counts):
    L = kzg.lib()
    cfg = kzg.make_config(tuning=tuning) if tuning else None
    rnd = random.Random(11)
    pool = CASES[:6] + rnd.sample(CASES, 300)
    for n in counts:
        vals = [pool[(3 * i + n) % len(pool)] for i in range(n)]
        sc = fr_bulk(kzg, vals)
        out1, out2 = (kzg.BlstP1 * (n + 1))(), (kzg.BlstP2 * (n + 1))()
        C.memset(out1, 0xa7, C.sizeof(out1))
        C.memset(out2, 0xa7, C.sizeof(out2))
        assert L.kzgamd_g1_mul_batch(out1, None, sc, n, C.byref(cfg) if cfg else None) == 0
        assert L.kzgamd_g2_mul_batch(out2, None, sc, n, C.byref(cfg) if cfg else None) == 0
        # nothing past the n-th output is written (for n = 0: nothing at all)
        assert bytes(out1)[144 * n:] == b"\xa7" * 144 and bytes(out2)[288 * n:] == b"\xa7" * 288, n
        assert_g1(out1, g1_expected("gen", vals), "n = %d" % n)
        assert_g2(kzg, out2, g2_expected(kzg, "gen", vals), "n = %d" % n)


def test_tuning_takes_mul_slice_alone(kzg):
    L = kzg.lib()
    sc = fr_bulk(kzg, [5])
    out1, out2 = (kzg.BlstP1 * 1)(), (kzg.BlstP2 * 1)()
    for bad in ("mul_slice=63", "mul_slice=32", "no_such_key=1", "spl=1"):
        cfg = kzg.make_config(tuning=bad)
        assert L.kzgamd_g1_mul_batch(out1, None, sc, 1, C.byref(cfg)) == -2, bad
        assert L.kzgamd_g2_mul_batch(out2, None, sc, 1, C.byref(cfg)) == -2, bad
        assert L.kzgamd_generate_trusted_setup(None, out1, None, None, 1, 0, bytes(32), C.byref(cfg)) == -2, bad
    cfg = kzg.make_config(tuning="mul_slice=64")
    assert L.kzgamd_g1_mul_batch(out1, None, sc, 1, C.byref(cfg)) == 0
    assert_g1(out1, g1_expected("gen", [5]), "mul_slice=64")
    assert "mul_slice" not in kzg.tuning_keys()
    with pytest.raises(kzg.KzgAmdError):
        kzg.FFTSettings(4, kzg.make_config(tuning="mul_slice=64"))
    info = kzg.group_mul_info()
    assert info["slice_points"] >= 64 and info["g1_window_bits"] >= 2 and info["g2_window_bits"] >= 2
