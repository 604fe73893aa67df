"""What the variable-base MSM engine (rust-kzg_amd/csrc/msm.hip) does with a given list of scalars, restated in plain
Python, and scalar lists built so that a chosen bucket has a chosen size at a chosen offset (TEST INFRASTRUCTURE).

The engine's control flow depends on the distribution of the scalars: a bucket of more than HEAVY entries is flagged and
its pieces (one per 2^lgc consecutive sorted entries it touches) are summed by whole waves, HSEG pieces per wave in a
first pass and the segment sums in a second.  With the endomorphism split off (tuning key glv=0) a scalar

    s = d * sum_{w < J} 2^(c w),    1 <= d <= 2^(c-1),

has the signed digit d in each of its first J windows and no carries, so a group of m points sharing it is a bucket of
exactly m entries (bucket d - 1) in each of the first J bucket sets, and the groups in digit order fix every offset.
The expected MSM of such a list needs no Pippenger: sum_j [s_j] (sum of the points of group j).

plan() restates the recoding, the sort's offsets and the piece geometry; the case builders return the scalars, the kind
of base per index and the groups; expected() is the group-sum reference on the oracle's point arithmetic.  The CPU module
(test_msm_bucket_edges_cpu.py) holds the constants below to the source and every case to the edge it is named after; the
GPU module (test_msm_bucket_edges_gpu.py) runs the cases."""
import ctypes as C
import random
from collections import namedtuple

# constants of msm.hip (test_msm_bucket_edges_cpu.py reads them out of the source and fails when they differ)
HEAVY = 512          # a bucket with MORE entries is flagged
HSEG = 1024          # pieces a wave sums in k_heavy's first pass
K_HEAVY_GRID_X = 256  # workgroups of pass 1 along the list of heavy buckets: more heavy buckets take the grid-stride loop
USE_TOP_MAX_SETS = 64  # more bucket sets in a launch: the plain (A, M) tree, k_level<true> with load_bucket
LANE_TARGET = 118000   # accumulation lanes a launch wants (eff_lgc's target = LANE_TARGET / sets of the launch)
# (smallest n, lgc) of the host's choice, first match wins; lgc_lo restates the line below it in msm.hip
LGC_BY_SIZE = ((1 << 22, 8), (1 << 20, 7), (1 << 19, 6), (1 << 18, 5), (0, 4))

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab


def default_lgc(n):
    """(lgc, lgc_lo) the host picks for an MSM of n points (no lgc tuning key)"""
    lgc = next(l for lim, l in LGC_BY_SIZE if n >= lim)
    return lgc, (lgc - 2 if lgc > 6 else (4 if lgc > 4 else lgc))


def eff_lgc(total, lo, hi, target):
    """the chunk a set of `total` entries takes on the device (eff_lgc in msm.hip)"""
    l = hi
    while l > lo and (total >> l) < target:
        l -= 1
    return l


def nwin_for(c):
    """windows of a 255-bit scalar without the endomorphism split"""
    return 255 // c + 1


def signed_digits(s, c, nwin):
    """k_digits / scalar_entries: d = low c bits + carry; d > 2^(c-1) -> d - 2^c and a carry into the next window
    (d == 2^(c-1) stays positive)"""
    half, mask, carry, out = 1 << (c - 1), (1 << c) - 1, 0, []
    for w in range(nwin):
        if not s and not carry:  # nothing left: the remaining digits are zero
            return out + [0] * (nwin - w)
        d = (s & mask) + carry
        s >>= c
        carry = 0
        if d > half:
            d -= 1 << c
            carry = 1
        out.append(d)
    return out


def structured_scalar(d, c, J):
    assert 1 <= d <= 1 << (c - 1)
    return d * sum(1 << (c * w) for w in range(J))


Bucket = namedtuple("Bucket", "bucket count beg end t0 t1 pieces heavy segments lgc")


def plan(scalars, live_mask, c, nwin, lgc, prepared=False, rows=None, heavy=HEAVY, hseg=HSEG):
    """Per bucket set: {"total", "lgc", "counts": {bucket: entries}, "buckets": [Bucket, ...] in bucket order}.
    lgc: an int, or a function of the set's total (eff_lgc).  live_mask[i] false: base i is infinity, no entries.
    prepared: one set shared by all windows (`rows` of them, default nwin), an entry per non-zero digit."""
    nw = (rows or nwin) if prepared else nwin
    nsets = 1 if prepared else nwin
    counts = [dict() for _ in range(nsets)]
    # distinct scalars once each (signed_digits), then their multiplicities: equal scalars are what the cases are made of
    mult = {}
    for s, live in zip(scalars, live_mask):
        if live and s:
            mult[s] = mult.get(s, 0) + 1
    for s, m in mult.items():
        for w, d in enumerate(signed_digits(s, c, nw)):
            if d:
                cs = counts[0 if prepared else w]
                b = abs(d) - 1
                cs[b] = cs.get(b, 0) + m
    sets = []
    for cs in counts:
        total = sum(cs.values())
        l = lgc(total) if callable(lgc) else lgc
        pos, bl = 0, []
        for b in sorted(cs):
            n = cs[b]
            beg, end = pos, pos + n
            t0, t1 = beg >> l, (end - 1) >> l
            pieces = t1 - t0 + 1
            bl.append(Bucket(b, n, beg, end, t0, t1, pieces, n > heavy, -(-pieces // hseg), l))
            pos = end
        sets.append({"total": total, "lgc": l, "counts": cs, "buckets": bl})
    return sets


def heavy_buckets(sets):
    return [b for s in sets for b in s["buckets"] if b.heavy]


# ---------------------------------------------------------------- cases
# kinds of base: DISTINCT keeps the generated point; (REPEAT, j) / (NEGATED, j): the point generated at index j / its
# negative; INF: (0, 0)
DISTINCT, REPEAT, NEGATED, INF = "distinct", "repeat", "negated", "inf"
Group = namedtuple("Group", "digit scalar start count")
Case = namedtuple("Case", "name c J lgc n scalars kinds groups nbatch")
# scalars: nbatch * n ints (MSM after MSM); kinds: n entries (bases are shared by the MSMs of a batch); groups: per MSM


class _Builder:
    """groups in digit order; pos = entries of a bucket set so far (every set of the first J looks the same; the rows
    engine's one shared set gets J entries per live point)"""
    per_row = False

    def __init__(self, c, J):
        self.c, self.J, self.pos, self.scalars, self.kinds, self.groups = c, J, 0, [], [], []

    def _per(self, J):
        return (self.J if J is None else J) if self.per_row else 1

    def group(self, m, d, J=None, kinds=None):
        s = structured_scalar(d, self.c, self.J if J is None else J)
        assert m >= 1 and (not self.groups or d > self.groups[-1].digit), "groups are listed in digit order"
        start = len(self.scalars)
        self.groups.append(Group(d, s, start, m))
        self.scalars += [s] * m
        ks = kinds(start, m) if kinds else [DISTINCT] * m
        self.kinds += ks
        self.pos += sum(k != INF for k in ks) * self._per(J)
        return self

    def align(self, d, C, more_than=0, J=None):
        """a group that ends exactly at a chunk end, of more than `more_than` entries (at least one point)"""
        m = 1
        while (self.pos + m * self._per(J)) % C or m * self._per(J) <= more_than:
            m += 1
        return self.group(m, d, J)

    def case(self, name, lgc, n=None, nbatch=1):
        n = n or len(self.scalars)
        pad = n - len(self.scalars)
        assert pad >= 0
        return Case(name, self.c, self.J, lgc, n, self.scalars + [0] * pad, self.kinds + [DISTINCT] * pad, [self.groups], nbatch)


def _last_inf(start, m):
    return [DISTINCT] * (m - 1) + [INF]


def case_threshold(H=HEAVY, S=HSEG, C=16, c=11, J=3):
    """buckets of H - 1, H, H + 1 entries, and one of H + 1 of which one base is infinity (H live entries) in the last
    bucket of the set (digit == half: the tie of the signed digits)"""
    half = 1 << (c - 1)
    b = _Builder(c, J)
    b.group(H - 1, 1).group(H, 7).group(H + 1, max(8, half * 300 // 1024)).group(H + 1, half, kinds=_last_inf)
    return b.case("threshold", None)


def case_alignment(H=HEAVY, S=HSEG, C=16, c=11, J=3):
    """heavy buckets that begin 1 and C - 1 entries after a chunk start and whose last piece holds one entry, one that
    ends exactly at a chunk end, and one in the last bucket that begins exactly on a chunk start"""
    half = 1 << (c - 1)
    b = _Builder(c, J)
    d = 1
    for a in (1, C - 1):
        b.group(a, d).group(H + C + 1 - a, d + 1).align(d + 2, C, more_than=H)
        d += 3
    b.group(H + 1, half)
    return b.case("alignment", None)


def _segment_groups(b, S, C, kinds=(None, None, None, None)):
    b.group(S * C, 1, kinds=kinds[0])               # S pieces: one segment, full
    b.group(S * C + 1, 2, kinds=kinds[1])           # S + 1 pieces: a second segment of one element
    b.align(3, C)                                    # (3 entries at the stated sizes)
    b.group(2 * S * C + 1, 4, kinds=kinds[2])       # 2 S + 1 pieces: three segments
    b.align(5, C)
    b.group(1, 6)
    b.group(S * C, 7, kinds=kinds[3])               # begins one entry after a chunk start: S + 1 pieces from S C entries
    return b


def case_segments(H=HEAVY, S=HSEG, C=4, c=11, J=3, lgc=2):
    """lgc = 2: buckets of exactly S, S + 1 and 2 S + 1 pieces (one, two, three segments of k_heavy's first pass), and S C
    entries that take S + 1 pieces because they begin one entry after a chunk start"""
    assert C == 1 << lgc
    return _segment_groups(_Builder(c, J), S, C).case("segments", lgc)


def case_segments_default_chunk(H=HEAVY, S=HSEG, C=16, c=11, J=3, n=1 << 15, one_bin=False):
    """the default chunk at n = 2^15 (two-level sort): a bucket of C S + 1 entries (S + 1 pieces), twenty of H + 1 on
    digits below 128 and one in the last bucket; one_bin: that one on a digit below 128 too, so that every entry of a
    set falls into the first coarse bin of the two-level sort"""
    half = 1 << (c - 1)
    b = _Builder(c, J)
    b.group(C * S + 1, 1)
    for k in range(20):
        b.group(H + 1, 2 + k)
    b.group(H + 1, min(100, half - 1) if one_bin else half)
    return b.case("segments_default_chunk" + ("_one_bin" if one_bin else ""), None, n=n)


def case_many_heavy(H=HEAVY, S=HSEG, C=16, c=11, J=11):
    """24 heavy buckets in each of 11 sets: 264 in the launch, more than the 256 workgroups of k_heavy's first pass"""
    half = 1 << (c - 1)
    b = _Builder(c, J)
    for k in range(24):
        b.group(H + 1, 1 + k * max(1, (half - 1) // 24))
    return b.case("many_heavy", None)


def _exceptional_kinds(variant, seed):
    """the bases of a group: (0) one point P repeated; (1) P and -P in equal numbers (the odd one out is infinity), so
    that the bucket sums to infinity; (2) P and -P with a surplus of 3; (3) as (2), with every fifth base infinity.  The
    signs are shuffled, so a chunk sums to a small multiple of P: equal pieces, opposite pieces and infinities for
    k_heavy's tree, doublings and cancellations inside k_accum's chain."""
    def kinds(start, m):
        rnd = random.Random(seed * 1000 + start)
        if variant == 0:
            return [DISTINCT] + [(REPEAT, start)] * (m - 1)
        idx = list(range(m))
        out = [None] * m
        if variant == 3:
            for i in idx[4::5]:
                out[i] = INF
            idx = [i for i in idx if out[i] is None]
        surplus = 0 if variant == 1 else 3
        if (len(idx) - surplus) % 2:
            out[idx.pop()] = INF
        npos = (len(idx) + surplus) // 2
        signs = [(REPEAT, start)] * npos + [(NEGATED, start)] * (len(idx) - npos)
        rnd.shuffle(signs)
        for i, k in zip(idx, signs):
            out[i] = k
        return out
    return kinds


def exceptional_multiple(kinds):
    """the multiple of P a group's bases sum to"""
    return sum(1 if k == DISTINCT or k[0] == REPEAT else -1 for k in kinds if k != INF)


def case_exceptional(rot, H=HEAVY, S=HSEG, C=4, c=11, J=3, lgc=2):
    """the group sizes of `segments` with the bases of the four multi-piece buckets replaced by +-P / infinity: variant
    (rot + k) % 4 on the k-th of them, so that the four values of rot put every variant on every bucket shape"""
    ks = [_exceptional_kinds((rot + k) % 4, 7 + rot) for k in range(4)]
    return _segment_groups(_Builder(c, J), S, C, ks).case("exceptional_%d" % rot, lgc)


def case_batch3(H=HEAVY, S=HSEG, C=4, c=13, J=3, lgc=2):
    """three MSMs over one handle (c = 13: 3 x 20 = 60 bucket sets, the top-of-tree forms): `segments`; all-zero scalars;
    one scalar for all n points"""
    seg = _segment_groups(_Builder(c, J), S, C).case("x", lgc)
    n = seg.n
    s = structured_scalar(5, c, J)
    return Case("batch3", c, J, lgc, n, seg.scalars + [0] * n + [s] * n, seg.kinds, [seg.groups[0], [], [Group(5, s, 0, n)]], 3)


def case_batch70(H=HEAVY, S=HSEG, C=4, c=11, J=3, lgc=2, nbatch=70):
    """seventy MSMs (more than 64 bucket sets: the plain tree, k_level<true> with load_bucket): in each a bucket of
    S C + 1 entries and a few small ones, on digits that differ from MSM to MSM"""
    half = 1 << (c - 1)
    scalars, groups, n = [], [], None
    for m in range(nbatch):
        b = _Builder(c, J)
        d0 = 1 + (m * 13) % (half - 12)
        b.group(3 + m % 5, d0).group(S * C + 1, d0 + 1 + m % 3).group(H // 8 + 1, d0 + 5).group(1 + m % 2, d0 + 11)
        cs = b.case("x", lgc, n=S * C + H // 8 + 16)
        n = cs.n
        scalars += cs.scalars
        groups.append(cs.groups[0])
    return Case("batch70", c, J, lgc, n, scalars, [DISTINCT] * n, groups, nbatch)


def case_rows_engine(H=HEAVY, S=HSEG, C=4, c=11, lgc=2):
    """a prepared handle without a wide table: one bucket set for all windows, a point has one entry per non-zero digit
    (J per group: 1, 2 or 3 windows), so that m J entries cross H and S C"""
    half = 1 << (c - 1)
    b = _Builder(c, 1)
    b.per_row = True
    b.group(H - 1, 1, J=1).group(H, 2, J=1).group(H + 1, 3, J=1).group(H + 1, 4, J=1, kinds=_last_inf)
    b.align(5, C, J=1)
    b.group(S * C // 2, 6, J=2)                 # S C entries on a chunk start: S pieces
    b.group(S * C + 1, 7, J=1)                  # S + 1 pieces
    b.align(8, C, J=1)
    b.group((2 * S * C + 3) // 3, half, J=3)    # >= 2 S C + 1 entries: three segments, in the last bucket
    return b.case("rows_engine", lgc)


def case_mixed_chunk(n=1 << 18, c=16, equal=32 * HSEG + 1, seed=5):
    """n = 2^18, 16-bit windows: half of the scalars random below 2^128, so that the upper bucket sets hold about half as
    many entries as the lower ones and take the smaller chunk (eff_lgc: 4 instead of 5); `equal` points share one
    full-length scalar — a multi-segment bucket in every set, under either chunk — the rest are random full-length."""
    rnd = random.Random(seed)
    nw = nwin_for(c)
    while True:
        s_eq = rnd.getrandbits(254)
        if s_eq < R and all(signed_digits(s_eq, c, nw)):
            break
    scalars = []
    for i in range(n):
        if i < equal:
            scalars.append(s_eq)
        elif i % 2:
            scalars.append(rnd.getrandbits(128))
        else:
            scalars.append(rnd.getrandbits(254))
    return Case("mixed_chunk", c, nw, None, n, scalars, [DISTINCT] * n, [None], 1)


def exceptional_cases():
    return [case_exceptional(r) for r in range(4)]


def all_structured_cases():
    """every case whose reference is expected(); builders called with the engine's constants"""
    return [case_threshold(), case_alignment(), case_segments(), case_segments_default_chunk(),
            case_segments_default_chunk(one_bin=True), case_many_heavy()] + exceptional_cases() + \
           [case_batch3(), case_batch70(), case_rows_engine()]


# ---------------------------------------------------------------- bases and the reference
def live_mask(case):
    return [k != INF for k in case.kinds]


def scalar_bytes(case):
    """canonical little-endian scalars, MSM after MSM"""
    return b"".join(s.to_bytes(32, "little") for s in case.scalars)


def materialise(case, raw):
    """raw: n x 96 bytes of blst_p1_affine (Montgomery limbs, little-endian) -> the same with the repeated, negated and
    infinity bases written over the generated ones.  -y is p - y in the Montgomery domain as well."""
    out = bytearray(raw)
    assert len(out) == 96 * case.n
    for i, k in enumerate(case.kinds):
        if k == DISTINCT:
            continue
        if k == INF:
            out[96 * i:96 * i + 96] = bytes(96)
            continue
        src = raw[96 * k[1]:96 * k[1] + 96]
        if k[0] == NEGATED:
            y = int.from_bytes(src[48:], "little")
            src = src[:48] + ((P - y) % P).to_bytes(48, "little")
        out[96 * i:96 * i + 96] = src
    return bytes(out)


def expected(groups, points, L, O, sums=None):
    """sum over the groups of [scalar] (sum of the group's points), on the oracle's point arithmetic (og1_*), compressed.
    points: ctypes array of oracle G1Affine after materialise(); sums: an optional dict that keeps the group sums
    (keyed by the group's index range) for MSMs of a batch that share groups."""
    total = O.G1()
    C.memset(C.byref(total), 0, C.sizeof(total))
    for g in groups:
        key = (g.start, g.count)
        acc = sums.get(key) if sums is not None else None
        if acc is None:
            acc = O.G1()
            C.memset(C.byref(acc), 0, C.sizeof(acc))
            t = O.G1()
            for i in range(g.start, g.start + g.count):
                L.og1_from_affine(C.byref(t), C.byref(points[i]))
                L.og1_add_or_dbl(C.byref(acc), C.byref(acc), C.byref(t))
            if sums is not None:
                sums[key] = acc
        term = O.G1()
        k = O.fr_from_int(g.scalar)
        L.og1_mul(C.byref(term), C.byref(acc), C.byref(k))
        L.og1_add_or_dbl(C.byref(total), C.byref(total), C.byref(term))
    buf = C.create_string_buffer(48)
    L.og1_compress(buf, C.byref(total))
    return buf.raw
