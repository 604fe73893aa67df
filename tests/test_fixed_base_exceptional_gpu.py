"""Exceptional point additions on every fixed-base MSM path: equal, opposite and infinite operands driven into each
accumulation and fold kernel of the wide-table engine (msm.hip: k_fbw_accum<SPL>, k_fbw_accum_quad, k_wide_tree,
k_wide_fold64, k_blocksum_hybrid, k_blocksum, k_lane_sum) and into the bucket engine of a prepared handle without a
wide table.

Every base is one of P, -P, 2P or infinity for ONE random point P, so the expected value of an MSM needs no MSM:
(sum of s_i * a_i mod r) * P with a_i in {1, -1, 2, 0} — Python integers and one og1_mul.  The scalar patterns make
collisions happen by symmetry, without a model of the lane layout:
  sym     s on P, r - s on -P: every lane partial sum of one GLV half is the same point, so the strided first fold
          level and every tree level / workgroup hand-over above it add equal operands (the doubling branch);
  cancel  the same s on P and -P: neighbouring partial sums are exact negatives (P + (-P) -> infinity) and
          infinities meet above them;
  half    cancel on one half of the indices, random scalars on the other: subtrees of infinity meet finite ones
          (inf + X), and within one launch some waves take the exceptional branches and others do not;
  digit   sym / cancel with s = m * 2^(c*w) (or that times X2 = x^2: the second GLV half), a single non-zero signed
          digit: every scalar of a lane's chain selects the same table entry (or its negative), so with two or more
          scalars per lane consecutive mixed additions of k_fbw_accum meet equal (doubling) or opposite (infinity)
          operands.  With one scalar per lane a chain holds one base, and a balanced signed-digit chain never
          collides with itself: those collisions exist only for spl >= 2;
  flip    sym with a sign that alternates over blocks of 32 indices (Thue-Morse): partial sums of two or more scalars
          per lane meet their exact negatives in the folds (a plain cancel pattern cancels inside such lanes);
  windows random digits in the windows of one quarter / two quarters of a GLV half only (chains of
          k_fbw_accum_quad that stay at infinity for most windows, partial sums at infinity next to finite ones);
plus scalars 0, 1, r - 1, (r -+ 1) / 2 and bases at infinity or 2P with non-zero scalars."""
import ctypes as C
import random

import pytest

import oracle_ffi as O

pytestmark = pytest.mark.gpu

N = 4096
X2 = 0xD201000000010000 ** 2  # the GLV split's divisor: k = k1 + k2 * X2 (glv.hip.h)
INF = b"\xc0" + bytes(47)
MONT = (1 << 256) % O.R
SPECIAL = range(4032, 4064)  # 2P (i % 4 < 2) and infinity (else) instead of the alternating +-P


def base_kind(i):
    if i in SPECIAL:
        return 2 if i % 4 < 2 else 0
    return 1 if i % 2 == 0 else -1


KIND = [base_kind(i) for i in range(N)]


def mont_bytes(vals):
    """blst_fr (Montgomery form) of canonical integers, as the host-buffer entry points take them"""
    return b"".join((v * MONT % O.R).to_bytes(32, "little") for v in vals)


def raw_bytes(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def compressed(L, p):
    g = O.G1()
    C.memmove(C.byref(g), C.byref(p) if not isinstance(p, (bytes, bytearray)) else p, 144)
    buf = C.create_string_buffer(48)
    L.og1_compress(buf, C.byref(g))
    return buf.raw


class Points:
    """P, -P, 2P (affine) for one random P, and (k * P) compressed for the expected values"""

    def __init__(self, L, seed):
        self.L = L
        g = O.G1()
        L.og1_generator(C.byref(g))
        self.p = O.G1()
        L.og1_mul(C.byref(self.p), C.byref(g), C.byref(O.fr_from_int(random.Random(seed).randrange(1, O.R))))
        self.aff = {}
        for a in (1, -1, 2):
            t = O.G1()
            L.og1_mul(C.byref(t), C.byref(self.p), C.byref(O.fr_from_int(a % O.R)))
            self.aff[a] = O.G1Affine()
            L.og1_to_affine(C.byref(self.aff[a]), C.byref(t))
        self.aff[0] = O.G1Affine()  # all-zero = infinity

    def bases(self, kinds):
        return (O.G1Affine * len(kinds))(*[self.aff[a] for a in kinds])

    def times(self, k):
        t = O.G1()
        self.L.og1_mul(C.byref(t), C.byref(self.p), C.byref(O.fr_from_int(k % O.R)))
        return compressed(self.L, t)


def expected_k(vals, kinds):
    return sum(v * a for v, a in zip(vals, kinds)) % O.R


# ---- scalar patterns over bases of the given kinds ----

def sym(s, kinds):
    return [(O.R - s) % O.R if a == -1 else s for a in kinds]


def cancel(s, kinds):
    return [0 if a == 2 else s for a in kinds]  # -> infinity: +-P pairs cancel, 2P gets 0, infinity bases give nothing


def thue_morse(b):
    return -1 if bin(b).count("1") % 2 else 1


def flip(s, kinds, block):
    """s * sign(i) * P per index, the sign a Thue-Morse sequence over blocks of `block` indices: two blocks whose numbers
    differ in one bit have opposite signs, so wherever a fold pairs lanes a power of two apart (strided first level,
    tree levels), the partial sums of lanes with two or more scalars meet their exact negatives"""
    inv2 = (O.R + 1) // 2
    out = []
    for i, a in enumerate(kinds):
        t = s if thue_morse(i // block) > 0 else (O.R - s) % O.R
        out.append((O.R - t) % O.R if a == -1 else t * inv2 % O.R if a == 2 else t)
    return out


def digit(m, w, c, second_half=False):
    v = m << (c * w)
    return v * X2 % O.R if second_half else v


def windows(rnd, c, wins, halves=(0,)):
    out = 0
    for h in halves:
        v = sum(rnd.randrange(1 << c) << (c * w) for w in wins) & ((1 << 126) - 1)
        out += v * X2 if h else v
    return out % O.R


def patterns(c, nwin, kinds, seed):
    """[(name, canonical scalars)] — the directed patterns, then one plain random MSM (always last)"""
    rnd = random.Random(seed)
    n = len(kinds)
    wmax = (126 - c) // c  # single digits stay below X2 / 2: the GLV split leaves them whole
    q = max(1, nwin // 4)
    pats = [
        ("sym_full", sym(rnd.randrange(1, O.R), kinds)),
        ("sym_small", sym(rnd.randrange(1, 1 << 100), kinds)),  # second GLV half zero: inf partial sums beside equal ones
        ("sym_digit_low", sym(digit(1, 0, c), kinds)),
        ("sym_digit_top", sym(digit(1 << (c - 1), wmax, c), kinds)),  # the largest digit: the last entry of a table row
        ("sym_digit_k2", sym(digit(5, 2, c, True), kinds)),
        ("cancel_full", cancel(rnd.randrange(1, O.R), kinds)),
        ("cancel_digit", cancel(digit(3, wmax // 2, c), kinds)),
        ("cancel_digit_k2", cancel(digit(1 << (c - 1), 1, c, True), kinds)),
        ("cancel_neg_digit", cancel(O.R - digit(7, 1, c), kinds)),
        ("flip_full", flip(rnd.randrange(1, O.R), kinds, 32)),
        ("flip_digit", flip(digit(9, 3, c), kinds, 32)),
        ("half_cancel_first", cancel(rnd.randrange(1, O.R), kinds)[: n // 2] + [rnd.randrange(O.R) for _ in range(n - n // 2)]),
        ("half_cancel_last", [rnd.randrange(O.R) for _ in range(n // 2)] + cancel(rnd.randrange(1, O.R), kinds)[n // 2:]),
        ("half_sym_last", [rnd.randrange(O.R) for _ in range(n // 2)] + sym(rnd.randrange(1, O.R), kinds)[n // 2:]),
        ("windows_one_quarter", [windows(rnd, c, range(q)) for _ in range(n)]),
        ("windows_last_quarter", [windows(rnd, c, range(nwin - q, nwin), (1,)) for _ in range(n)]),
        ("windows_two_quarters", [windows(rnd, c, list(range(q)) + list(range(2 * q, 3 * q)), (0, 1)) for _ in range(n)]),
    ]
    edge = [rnd.randrange(O.R) for _ in range(n)]
    for i in range(0, n, 5):
        edge[i] = [0, 1, O.R - 1, (O.R - 1) // 2, (O.R + 1) // 2][(i // 5) % 5]
    pats.append(("edge_scalars", edge))
    pats.append(("random", [rnd.randrange(O.R) for _ in range(n)]))
    return pats


# ---- module-wide state: one Points, the patterns per window size, one live wide-table handle ----

_state = {}


def points(oracle):
    if "pts" not in _state:
        _state["pts"] = Points(oracle.lib(), 0xFB0)
    return _state["pts"]


def prepared(kzg, oracle, tuning):
    """the 4096-point handle for (flavour, tuning): one live at a time (6.4 GB each)"""
    key = (kzg.__name__, tuple(sorted(tuning.items())))
    if _state.get("key") != key:
        if _state.get("h") is not None:
            _state["h"].close()
            _state["h"] = None
        P = points(oracle)
        h = kzg.prepare_multi_scalar_mult(P.bases(KIND), N, kzg.make_config(table_budget_gb=8.0, tuning=tuning))
        _state["h"], _state["key"] = h, key
    return _state["h"]


def pattern_set(oracle, c, nwin):
    """[(name, mont bytes, raw bytes, expected compressed)] for the 4096-point layout"""
    key = ("pats", c, nwin)
    if key not in _state:
        P = points(oracle)
        _state[key] = [(name, mont_bytes(v), raw_bytes(v), P.times(expected_k(v, KIND))) for name, v in patterns(c, nwin, KIND, 4096 + c)]
    return _state[key]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    if _state.get("h") is not None:
        _state["h"].close()
    _state.clear()


def launches(pats, nbatch):
    """batches of nbatch patterns that together cover every pattern; from two MSMs on, every batch has the random one"""
    directed, rand = pats[:-1], pats[-1]
    if nbatch == 1:
        return [[p] for p in pats]
    per = nbatch - 1
    out = []
    for k in range(-(-len(directed) // per)):
        b = [directed[(k * per + j) % len(directed)] for j in range(per)]
        b.insert(k % nbatch, rand)
        out.append(b)
    return out


def check_both_entry_points(kzg, L, h, n, batch):
    """host buffers (Montgomery scalars) and device buffers (raw scalars, caller's stream), each called twice — the device
    form with no synchronisation in between, so the second launch finds the fold counters where the first left them"""
    import torch

    nb = len(batch)
    want = [w for _, _, _, w in batch]
    names = [name for name, _, _, _ in batch]
    mont = b"".join(m for _, m, _, _ in batch)
    sc = (O.Fr * (n * nb)).from_buffer_copy(mont)
    for call in range(2):
        got = kzg.multi_scalar_mult_prepared_batch(h, sc, n, nb)
        bad = [names[b] for b in range(nb) if compressed(L, got[b]) != want[b]]
        assert not bad, ("host", call, bad)
    stream = torch.cuda.current_stream().cuda_stream
    d_sc = torch.frombuffer(bytearray(b"".join(r for _, _, r, _ in batch)), dtype=torch.uint8).cuda()
    outs = [torch.full((nb * 144,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    for d_out in outs:
        kzg.msm_prepared_batch_device(h, d_out.data_ptr(), d_sc.data_ptr(), n, nb, False, stream)
    torch.cuda.synchronize()
    for call, d_out in enumerate(outs):
        raw = d_out.cpu().numpy().tobytes()
        bad = [names[b] for b in range(nb) if compressed(L, raw[b * 144:(b + 1) * 144]) != want[b]]
        assert not bad, ("device", call, bad)


# Which kernels a (tuning, nbatch) pair reaches over 4096 points with a GLV table (msm_enqueue, the wide-table branch):
#   {}                1, 2, 4: k_fbw_accum_quad + k_wide_tree; 5, 8: k_fbw_accum<1> + k_blocksum_hybrid;
#                     17: k_fbw_accum<2> + k_blocksum_hybrid; 256: k_fbw_accum<8> + k_blocksum (128 threads)
#   quad_accum_max=0  1, 2, 4: k_fbw_accum<1> + k_wide_tree
#   no_wide_tree=1    1, 2, 4: k_fbw_accum_quad + two launches of k_wide_fold64
#   no_hybrid_fold=1  5, 8: two launches of k_blocksum; 17: one of 256 threads
#   no_wide_tail=1    k_fbw_accum<2> (no spl = 1 lane form, no quad) + k_blocksum only
#   spl=2 / 4 / 16    k_fbw_accum<4> / <8> / <32> (2048 / 1024 / 256 partial sums) + k_blocksum
#   blocksum_threads  k_blocksum of 64 / 128 threads for the batches that fold in one launch (256)
TUNINGS = [{}, {"quad_accum_max": 0}, {"no_wide_tree": 1}, {"no_hybrid_fold": 1}, {"no_wide_tail": 1}, {"spl": 2}, {"spl": 4},
           {"spl": 16}, {"blocksum_threads": 64}, {"blocksum_threads": 128}]


@pytest.mark.parametrize("nbatch", [1, 2, 4, 5, 8, 17, 256])
@pytest.mark.parametrize("tuning", TUNINGS, ids=lambda t: ";".join("%s=%d" % kv for kv in t.items()) or "default")
def test_wide_table_exceptional_additions(oracle, kzg, tuning, nbatch):
    L = oracle.lib()
    h = prepared(kzg, oracle, tuning)
    info = h.info()
    assert info["wide_table"] and info["wide_glv"], info
    pats = pattern_set(oracle, info["window_bits"], info["rows"])
    assert all(w == INF for name, _, _, w in pats if name.startswith("cancel"))
    for batch in launches(pats, nbatch):
        check_both_entry_points(kzg, L, h, N, batch)


def test_montgomery_packing_matches_the_oracle(oracle):
    """the Python-side Montgomery packing the tests above feed the host entry points"""
    for v in (0, 1, 2, O.R - 1, X2, (O.R + 1) // 2, 0x1234567890ABCDEF << 130):
        assert mont_bytes([v]) == bytes(O.fr_from_int(v)), hex(v)


# ---- the matrix handle (FK20 shape: MSMs of 64 table bases, segment accumulation + k_lane_sum) ----

ROWS, COLS = 128, 64


def matrix_kind(r, c):
    layout = r % 4
    if layout == 0:
        return 1
    if layout == 1:
        return 1 if c % 2 == 0 else -1
    if layout == 2:
        return 0 if c % 16 == 5 else (1 if c % 2 == 0 else -1)
    return 0 if c == COLS - 1 else -1


def matrix_row_scalars(rnd, kinds, form, cbits):
    s = rnd.randrange(1, O.R)
    d = digit(1 + rnd.randrange(1 << (cbits - 1)), rnd.randrange(4), cbits, rnd.randrange(2) == 1)
    if form == 0:
        return sym(s, kinds)
    if form == 1:
        return sym(d, kinds)
    if form == 2:
        return cancel(d, kinds)
    if form == 3:
        return cancel(s, kinds)
    if form == 4:
        return cancel(s, kinds)[: COLS // 2] + [rnd.randrange(O.R) for _ in range(COLS // 2)]
    if form == 5:
        return [0] * COLS
    if form == 8:
        return flip(s, kinds, 8)
    if form == 9:
        return flip(d, kinds, COLS // 2)
    if form == 6:
        v = [rnd.randrange(O.R) for _ in range(COLS)]
        v[0], v[1], v[2] = 0, 1, O.R - 1
        return v
    return [windows(rnd, cbits, range(2)) for _ in range(COLS)]


# nmat 1: 128 segment MSMs, two scalars per lane (k_fbw_accum<2>); nmat 2: 256 MSMs, spl 4 (k_fbw_accum<8>);
# spl = 8 / 16: k_fbw_accum<16> / <32> — 8 / 4 partial sums per MSM; every form folds with k_lane_sum
@pytest.mark.parametrize("nmat,tuning", [(1, {}), (2, {}), (1, {"spl": 8}), (2, {"spl": 16})],
                         ids=["nmat1", "nmat2", "nmat1-spl=8", "nmat2-spl=16"])
def test_matrix_exceptional_additions(oracle, kzg, nmat, tuning):
    L = oracle.lib()
    P = points(oracle)
    kinds = [matrix_kind(r, c) for r in range(ROWS) for c in range(COLS)]
    h = kzg.MatrixMsm(P.bases(kinds), ROWS, COLS, kzg.make_config(table_budget_gb=16, tuning=tuning))
    try:
        info = h.info()
        assert info["wide_table"] and info["wide_glv"], info
        rnd = random.Random(12864 + nmat)
        vals, want = [], []
        for k in range(nmat * ROWS):
            row = kinds[(k % ROWS) * COLS:(k % ROWS + 1) * COLS]
            v = matrix_row_scalars(rnd, row, (k // 4 + 3 * (k % 4)) % 10, info["window_bits"])  # every form on every layout
            vals += v
            want.append(P.times(expected_k(v, row)))
        sc = (O.Fr * len(vals)).from_buffer_copy(mont_bytes(vals))
        for call in range(2):
            out = h.multiply_batch(sc, nmat)
            bad = [k for k in range(nmat * ROWS) if compressed(L, out[k]) != want[k]]
            assert not bad, (call, bad)
        assert INF in want
    finally:
        h.close()


# ---- a prepared handle without a wide table: the fixed-base-rows bucket engine ----

@pytest.mark.parametrize("nbatch", [1, 17])
def test_prepared_rows_without_wide_table_exceptional_additions(oracle, kzg, nbatch):
    L = oracle.lib()
    P = points(oracle)
    h = kzg.prepare_multi_scalar_mult(P.bases(KIND), N, kzg.make_config(no_tables=True))
    try:
        info = h.info()
        assert not info["wide_table"] and info["rows"] > 1, info
        pats = pattern_set(oracle, 11, 12)  # the same scalars as the wide-table tests (digits of that table's windows)
        for batch in launches(pats, nbatch):
            check_both_entry_points(kzg, L, h, N, batch)
    finally:
        h.close()
