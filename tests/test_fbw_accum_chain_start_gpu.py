"""The start of a lane's chain in k_fbw_accum (msm.hip, g1::chain_add): the first table point is taken as it is, the
second is added affine + affine, and only then does the general mixed addition run — with zero digits, table slots of a
base at infinity, equal and opposite points and the end of a segment all able to fall on those first steps.

Wide tables over 5 and 8 bases, every base a small multiple of ONE random point P (0 = infinity), so an MSM's expected
value is (sum s_i * k_i mod r) * P: Python integers and one og1_mul.  With so few bases every lane is a chain start:
  batches of 1 and 3   k_fbw_accum<2, true>: a lane takes the k1 or k2 digits of two neighbouring scalars — 5 bases leave
                       the last lane one scalar and a segment end, 8 fill every lane;
  batches of 256       k_fbw_accum<8, true>: four scalars per lane were asked for, so one lane pair holds all 5 bases
                       (segment end inside the lane), or all 8 exactly;
  fbw_glv=0            the same over the plain 255-bit table: k_fbw_accum<1, false> and k_fbw_accum<4, false>.
Scalars: all zero; ONE non-zero signed digit (the same table entry from neighbouring bases: with equal scalars on
repeated bases the second point of a chain equals the first -> doubling; on negated bases it is its opposite ->
infinity, and the chain starts again); digits of both signs; zero first windows; a base at infinity in first and in
second place of a lane; r - 1; random."""
import ctypes as C
import random

import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

X2 = 0xD201000000010000 ** 2  # the GLV split's divisor: k = k1 + k2 * X2 (glv.hip.h)
MONT = (1 << 256) % O.R
# bases as multiples of P.  Lanes of two scalars pair them (0,1) (2,3) ..., lanes of four / eight take them in order.
LAYOUTS = {
    8: [[1, 1, -1, 1, 0, 1, 1, 0],      # repeated; negated; infinity first; infinity second
        [0, 0, 1, -1, 1, 1, 2, -2]],    # a lane of infinities; a long chain: inf, inf, P - P -> empty, P + P, 2P + 2P - 2P
    5: [[1, 1, -1, 0, 1],               # repeated; negated then infinity; a last lane with one scalar
        [0, 1, -1, 1, 1]],              # infinity first; negated; the same
}


def compressed(L, p):
    g = O.G1()
    C.memmove(C.byref(g), C.byref(p), 144)
    buf = C.create_string_buffer(48)
    L.og1_compress(buf, C.byref(g))
    return buf.raw


class Points:
    def __init__(self, L, seed):
        self.L = L
        g = O.G1()
        L.og1_generator(C.byref(g))
        self.p = O.G1()
        L.og1_mul(C.byref(self.p), C.byref(g), C.byref(O.fr_from_int(random.Random(seed).randrange(1, O.R))))
        self.aff = {0: O.G1Affine()}  # all-zero = infinity
        self.cache = {}

    def base(self, k):
        if k not in self.aff:
            t = O.G1()
            self.L.og1_mul(C.byref(t), C.byref(self.p), C.byref(O.fr_from_int(k % O.R)))
            self.aff[k] = O.G1Affine()
            self.L.og1_to_affine(C.byref(self.aff[k]), C.byref(t))
        return self.aff[k]

    def bases(self, kinds):
        return (O.G1Affine * len(kinds))(*[self.base(k) for k in kinds])

    def times(self, k):
        k %= O.R
        if k not in self.cache:
            t = O.G1()
            self.L.og1_mul(C.byref(t), C.byref(self.p), C.byref(O.fr_from_int(k)))
            self.cache[k] = compressed(self.L, t)
        return self.cache[k]


def digit(d, w, c, second_half=False):
    v = d << (c * w)
    return v * X2 % O.R if second_half else v


def windows_from(rnd, c, first, halves):
    """random digits in the windows first.. of the given GLV halves only: the windows below are zero"""
    out = 0
    for h in halves:
        v = (rnd.getrandbits(126) >> (c * first)) << (c * first)
        out += v * X2 if h else v
    return out % O.R


def patterns(n, c, seed):
    """[(name, scalars)]: the directed patterns, then random ones"""
    rnd = random.Random(seed)
    wmax = (126 - c) // c  # single digits stay below X2 / 2: the GLV split leaves them whole
    top = 1 << (c - 1)
    pats = [("zeros", [0] * n)]
    for w in (0, wmax // 2, wmax):
        for half in (False, True):
            for d in (1, 5, top):
                s = digit(d, w, c, half)
                tag = "digit%d_w%d_%s" % (d, w, "k2" if half else "k1")
                pats.append((tag, [s] * n))                              # equal scalars: doubling / cancellation at the start
                pats.append((tag + "_neg", [(O.R - s) % O.R] * n))       # the same through the sign of the table point
                pats.append((tag + "_alt", [s if i % 2 == 0 else (O.R - s) % O.R for i in range(n)]))
    one = digit(3, 1, c)
    pats.append(("digit_then_random", [one] + [rnd.randrange(O.R) for _ in range(n - 1)]))
    pats.append(("digit_zero_digit", [one if i % 2 == 0 else 0 for i in range(n)]))  # zero scalars between the points
    pats.append(("zero_then_digit", [0 if i % 2 == 0 else one for i in range(n)]))
    for first in (1, 3, wmax):
        pats.append(("first_%d_windows_zero" % first, [windows_from(rnd, c, first, (0, 1)) for _ in range(n)]))
        pats.append(("first_%d_windows_zero_k1_only" % first, [windows_from(rnd, c, first, (0,)) for _ in range(n)]))
    pats.append(("r_minus_1", [O.R - 1] * n))
    pats.append(("r_minus_1_and_1", [O.R - 1 if i % 2 == 0 else 1 for i in range(n)]))
    eq = rnd.randrange(1, O.R)
    pats.append(("equal_random", [eq] * n))
    for k in range(3):
        pats.append(("random%d" % k, [rnd.randrange(O.R) for _ in range(n)]))
    return pats


_state = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    if _state.get("h") is not None:
        _state["h"].close()
    _state.clear()


def handle(kzg, oracle, n, layout, glv):
    """one live handle at a time: (flavour, n, layout, form) -> wide table over the layout's bases"""
    key = (kzg.__name__, n, layout, glv)
    if _state.get("key") != key:
        if _state.get("h") is not None:
            _state["h"].close()
            _state["h"] = None
        if "pts" not in _state:
            _state["pts"] = Points(oracle.lib(), 0xC4A1)
        cfg = kzg.make_config(table_budget_gb=1.0, tuning={} if glv else {"fbw_glv": 0})
        _state["h"] = kzg.prepare_multi_scalar_mult(_state["pts"].bases(LAYOUTS[n][layout]), n, cfg)
        _state["key"] = key
    return _state["h"], _state["pts"]


def batches(pats, nbatch):
    """launches of nbatch MSMs that together hold every pattern"""
    if nbatch >= len(pats):
        return [[pats[i % len(pats)] for i in range(nbatch)]]
    return [[pats[(k + j) % len(pats)] for j in range(nbatch)] for k in range(0, len(pats), nbatch)]


@pytest.mark.parametrize("glv", [True, False], ids=["glv", "plain"])
@pytest.mark.parametrize("nbatch", [1, 3, 256])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("n", [5, 8])
def test_chain_starts_against_the_oracle(oracle, kzg, n, layout, nbatch, glv):
    L = oracle.lib()
    h, P = handle(kzg, oracle, n, layout, glv)
    info = h.info()
    assert info["wide_table"] and info["wide_glv"] == glv, info
    kinds = LAYOUTS[n][layout]
    pats = patterns(n, info["window_bits"], 1000 * n + layout)
    assert len(pats) < 256
    for batch in batches(pats, nbatch):
        vals = [v for _, sc in batch for v in sc]
        sc = (O.Fr * len(vals)).from_buffer_copy(b"".join((v * MONT % O.R).to_bytes(32, "little") for v in vals))
        got = kzg.multi_scalar_mult_prepared_batch(h, sc, n, nbatch)
        bad = [name for b, (name, s) in enumerate(batch)
               if compressed(L, got[b]) != P.times(sum(v * k for v, k in zip(s, kinds)))]
        assert not bad, bad
