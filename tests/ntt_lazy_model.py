"""Exact-integer model of the LAZY values inside the Fr transforms (ntt.hip, fr29.hip.h): which value reaches
reduce_lazy / finish (and, in the fused DAS extension, the twist) for a given input, and inputs built to drive that value
towards the bound the code relies on (< 64r).

The pass structure is the planner's (tools/ntt_plan_sim.py: split_passes, the DIT stage order, which stages are unit
stages): n <= 4096 is one pass of plan kind A1; above that a pass of kind A2 and then passes of kind B, with the
canonical residue between passes; the DAS extension of <= 4096 evens is the fused plan (inverse rounds, twist, forward
rounds).  Which thread holds which element does not change a value, so the model has no tiles: it works on the DIT
position array a[p] (a[p] = x[brev(p)] on entry, natural order on exit), at VALUE level:
    mul_signed(a, W)       = (a W - m r) / 2^261,  m = a W r^-1 mod 2^261        (in (-r, r) for a < 64r, W < r)
    butterfly_signed       x, y -> x + t + r,  x + 4r - t      t = mul_signed(y, W)
    butterfly_lazy  (unit) x, y -> x + y,      x + 4r - y      stage 0 of a first pass (w^0 = 1, no multiplication)
    butterfly_lazy8 (unit) x, y -> x + y,      x + 8r - y      stage 1 of a first pass, the pairs with twiddle w^0
Data is whatever the 32 bytes of an element hold (blst's Montgomery form, but the transform is linear: the model never
needs to know); twiddles are W = w 2^261 mod r, canonical, w the powers of 7^((r-1)/n).

AIMED INPUTS.  Output o of a pass of T stages is reached through the chain  q_s = o with the bits of stages >= s cleared:
stage s turns a[q_s] into a[q_s] + 4r - t (bit s of o set) or a[q_s] + t + r (clear), t = mul_signed(a[q_s | 2^s], W).
With t in (-r, r) congruent to rho = a w mod r, t = rho - r exactly when rho > a W / 2^261: the residue just above
a W / 2^261 gives t just above -r + a W / 2^261, and the step gains almost 5r.  a[q_s | 2^s] is the output of a
sub-transform over positions that no other stage of the chain reads, so ONE input per stage (at q_0 | 2^s, which that
sub-transform never multiplies) sets its residue; a few fixed-point steps settle rho against a, which depends on the
input chosen.  The other inputs (`fill`) may be anything: the builder takes their contribution out.  The path bound of
such a chain is  x0 + sum over stages of (5r if the bit is set else 2r)  with 4r (8r) instead of 5r at the unit stages:
for o = 2^T - 1 that is x0 + 4r + 5r (T - 1) in a first pass and x0 + 5r T in a pass of kind B; the value stays below it
by sum a_s W_s / 2^261.

Passes of kind B with T = 10 stages need n = 2^20: about 10^7 exact multiplications per run, too slow for this model —
out of scope; the longest kind-B pass modelled has 7 stages (n = 2^14)."""
import random

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
K = 261
MASK = (1 << K) - 1
RI = pow(R, -1, 1 << K)       # r^-1 mod 2^261
ONE = (1 << K) % R            # 2^261 mod r
INV = pow(1 << K, -1, R)      # 2^-261 mod r
LOGT = 12


def mul_signed(a, W):
    p = a * W
    return (p - ((p * RI) & MASK) * R) >> K


def brev(v, bits):
    r = 0
    for k in range(bits):
        if (v >> k) & 1:
            r |= 1 << (bits - 1 - k)
    return r


def split_passes(L):
    """stage counts per pass (tools/ntt_plan_sim.py, ntt_plan.h): one pass up to 4096, else balanced passes of <= 10"""
    if L <= LOGT:
        return [L]
    np_ = (L + 9) // 10
    base, extra = divmod(L, np_)
    return [base + (1 if i < extra else 0) for i in range(np_)]


_tw_cache = {}


def twiddles(L, inverse):
    """stage-major table as the kernels index it: entry (2^s - 1) + j = w_(2^(s+1))^(+-j) 2^261 mod r"""
    key = (L, inverse)
    if key not in _tw_cache:
        n = 1 << L
        w = pow(7, (R - 1) >> L, R) if L else 1
        if inverse:
            w = pow(w, -1, R)
        pw = [ONE]
        for _ in range(1, max(1, n // 2)):
            pw.append(pw[-1] * w % R)
        tab = []
        for s in range(L):
            tab += [pw[j * (n >> (s + 1))] for j in range(1 << s)]
        _tw_cache[key] = tab
    return _tw_cache[key]


def run_column(col, s0, nst, c, tw, first):
    """stages s0 .. s0 + nst - 1 on the positions c + (k << s0), k < len(col) (in place); first: the pass is a
    transform's first one (s0 = 0), whose stage 0 and the w^0 pairs of stage 1 are unit.  Returns the largest value."""
    top = 0
    m = len(col)
    for st in range(nst):
        half = 1 << st
        base = (1 << (s0 + st)) - 1 + c
        for blk in range(0, m, 2 * half):
            for j in range(half):
                i = blk + j
                x, y = col[i], col[i + half]
                if first and st == 0:
                    col[i], col[i + half] = x + y, x + 4 * R - y
                elif first and st == 1 and j == 0:
                    col[i], col[i + half] = x + y, x + 8 * R - y
                else:
                    t = mul_signed(y, tw[base + (j << s0)])
                    col[i], col[i + half] = x + t + R, x + 4 * R - t
                if col[i] > top:
                    top = col[i]
                if col[i + half] > top:
                    top = col[i + half]
    return top


def run_pass(a, L, s0, T, tw, first):
    """one pass over the whole position array: every column of every block of 2^(s0 + T) positions"""
    top = 0
    span = 1 << (s0 + T)
    for blk in range(0, 1 << L, span):
        for c in range(1 << s0):
            col = a[blk + c: blk + span: 1 << s0]
            top = max(top, run_column(col, s0, T, c, tw, first))
            a[blk + c: blk + span: 1 << s0] = col
    return top


def transform(x, L, inverse=False):
    """-> dict(reached = [per pass: the lazy values that reach reduce_lazy / finish, by position], top = the largest value
    anywhere in the run, out = the residues the transform returns)"""
    n = 1 << L
    tw = twiddles(L, inverse)
    a = [x[brev(i, L)] for i in range(n)]
    reached, top, s0 = [], 0, 0
    for pi, T in enumerate(split_passes(L)):
        top = max([top, run_pass(a, L, s0, T, tw, pi == 0)] + a)
        reached.append(list(a))
        a = [v % R for v in a]
        s0 += T
    if inverse:
        ninv = pow(n, -1, R)
        a = [v * ninv % R for v in a]
    return dict(reached=reached, top=top, out=a)


def das(evens, L):
    """the fused DAS extension of 2^L <= 4096 evens -> dict(reached = [what reaches the twist, what reaches finish],
    fwd_in = the forward half's lazy inputs by natural position (< 2r), top, out)"""
    n = 1 << L
    a = [evens[brev(i, L)] for i in range(n)]
    top = max([run_pass(a, L, 0, L, twiddles(L, True), True)] + a)
    w2 = pow(7, (R - 1) >> (L + 1), R)
    u, p = [], ONE
    for j in range(n):
        u.append(mul_signed(a[j], p) + R)
        p = p * w2 % R
    b = [u[brev(i, L)] for i in range(n)]
    top = max([top, run_pass(b, L, 0, L, twiddles(L, False), True)] + b)
    ninv = pow(n, -1, R)
    return dict(reached=[a, b], fwd_in=u, top=top, out=[v * ninv % R for v in b])


# ---------------------------------------------------------------------------------------------- plain references
def dft_fast(x, L, inverse=False, scale=True):
    """the textbook recursive transform on residues (no lazy values, no passes): what the model's `out` must equal"""
    n = 1 << L
    w = pow(7, (R - 1) >> L, R) if L else 1
    if inverse:
        w = pow(w, -1, R)

    def rec(v, wr):
        if len(v) == 1:
            return [v[0] % R]
        e, o = rec(v[0::2], wr * wr % R), rec(v[1::2], wr * wr % R)
        out, t, h = [0] * len(v), 1, len(v) // 2
        for i in range(h):
            y = o[i] * t % R
            out[i], out[i + h] = (e[i] + y) % R, (e[i] - y) % R
            t = t * wr % R
        return out

    out = rec(list(x), w)
    if inverse and scale:
        ninv = pow(n, -1, R)
        out = [v * ninv % R for v in out]
    return out


def dft_direct(x, L, outputs, inverse=False):
    """sum x_k w^(jk) for the listed outputs j only (the definition; O(n) each)"""
    n = 1 << L
    w = pow(7, (R - 1) >> L, R) if L else 1
    if inverse:
        w = pow(w, -1, R)
    res = {}
    for j in outputs:
        wj, t, acc = pow(w, j, R), 1, 0
        for k in range(n):
            acc += x[k] * t
            t = t * wj % R
        res[j] = acc * (pow(n, -1, R) if inverse else 1) % R
    return res


def das_reference(evens, L):
    """FFT_n(w_2n^j IFFT_n(evens)_j) on residues"""
    c = dft_fast(evens, L, inverse=True)
    w2, p = pow(7, (R - 1) >> (L + 1), R), 1
    for j in range(1 << L):
        c[j] = c[j] * p % R
        p = p * w2 % R
    return dft_fast(c, L)


# ---------------------------------------------------------------------------------------------- aimed inputs
def path_bound(x0, o, s0, T, first):
    """the bound of the chain to output o (module docstring), for a chain that starts from the value x0"""
    b = x0
    for st in range(T):
        bit = (o >> (s0 + st)) & 1
        if first and st == 0:
            b += 4 * R if bit else R                      # x + 4r - y  /  x + y, y < r
        elif first and st == 1 and not o & 1:
            b += 8 * R if bit else 2 * R                  # x + 8r - y  /  x + y, y < 2r
        else:
            b += 5 * R if bit else 2 * R
    return b


def aim_pass(o, s0, T, tw, first, x0, fill=0, seed=1, lazy_of=None):
    """pass-input values (position -> value, positions of the whole array) that drive output position o of the pass of
    stages s0 .. s0 + T - 1 towards its path bound; every other input of the pass is taken to be `fill`.
    lazy_of(position, residue) -> the lazy value the pass really reads for a chosen residue (the DAS forward half reads
    residue or residue + r); identity when None."""
    rnd = random.Random(seed)
    lazy_of = lazy_of or (lambda p, v: v)
    passmask = ((1 << T) - 1) << s0
    base, c = o & ~passmask, o & ((1 << s0) - 1)
    chosen = {base: x0}
    for st in range(T):
        s = s0 + st
        bit = (o >> s) & 1
        z = base | (1 << s)                       # the input that sets this stage's multiplicand
        idx = (o >> s0) & ((1 << st) - 1)         # where the multiplicand leaves its sub-transform

        def sub(v):
            col = [lazy_of(z + (k << s0), fill) for k in range(1 << st)]
            col[0] = lazy_of(z, v)
            run_column(col, s0, st, c, tw, first)
            return col[idx]

        if first and (st == 0 or (st == 1 and not o & 1)):
            # unit stage: y itself is subtracted (bit set: as small as possible) or added (as large as a canonical
            # value gets); the multiplicand's residue is v plus what the fill contributes
            offs = sub(0) % R
            chosen[z] = (-offs) % R if bit else (R - 1 - offs) % R
            if st == 1 and not bit:
                chosen[z + 1] = R - 1 if not fill else fill
            continue
        W = tw[(1 << s) - 1 + (o & ((1 << s) - 1))]
        winv = pow(W * INV % R, -1, R)
        offs = sub(0) % R                          # residue the fill alone leaves at idx (v adds itself: local 0 is never multiplied)
        best = None
        rho = 1
        for _ in range(8):
            v = (rho * winv - offs) % R
            a = sub(v)
            t = mul_signed(a, W)
            score = -t if bit else t
            if best is None or score > best[0]:
                best = (score, v)
            edge = a * W >> K                      # t = rho - r exactly for rho > edge
            rho = (edge + 1 + rnd.randrange(1 << 200)) if bit else max(0, edge - rnd.randrange(1 << 200))
        chosen[z] = best[1]
    return chosen


def random_top(L, shape, seeds=(1, 2, 3)):
    """the largest value that reaches reduce_lazy / finish over uniformly random canonical inputs; shape: "fwd", "inv",
    "das"; -> [per pass maximum]"""
    tops = None
    for sd in seeds:
        rnd = random.Random(1000 * L + sd)
        x = [rnd.randrange(R) for _ in range(1 << L)]
        res = das(x, L) if shape == "das" else transform(x, L, shape == "inv")
        m = [max(p) for p in res["reached"]]
        tops = m if tops is None else [max(a, b) for a, b in zip(tops, m)]
    return tops


# ---------------------------------------------------------------------------------------------- stored vectors
# A stored vector (tests/golden/ntt_worst_inputs.json, written by tests/golden/make_ntt_worst_inputs.py) is sparse:
#   shape "fwd" / "inv" / "das", logn, nbatch, fill (the value of every entry not listed), seed,
#   space: "input"    entries are inputs of the transform,
#          "boundary" entries are the canonical residues between the first pass and the second, by position: the inputs
#                     are the inverse of the first pass's blocks (exact, a few small transforms),
#          "fwd_half" entries are the residues the DAS forward half starts from, by natural position: the evens are
#                     n^-1 FFT(residue_j w_2n^-j),
#   entries [[transform, index, value]], targets [[transform, pass, output position]], reached [value per target].
def materialise(vec):
    """-> the inputs, one list of 2^logn integers per transform of the batch"""
    L, n = vec["logn"], 1 << vec["logn"]
    fill = int(vec["fill"], 16)
    rows = [[fill] * n for _ in range(vec["nbatch"])]
    for b, i, v in vec["entries"]:
        rows[b][i] = int(v, 16)
    if vec["space"] == "boundary":
        TA = split_passes(L)[0]
        out = []
        for row in rows:
            a = [0] * n
            for blk in range(0, n, 1 << TA):
                seg = row[blk: blk + (1 << TA)]
                if any(seg):
                    # the first pass computes, block by block, the 2^TA-point transform with the root w_n^(2^(L - TA))
                    a[blk: blk + (1 << TA)] = [seg_in for seg_in in _block_inverse(seg, TA, vec["shape"] == "inv")]
            out.append([a[brev(i, L)] for i in range(n)])  # a[p] = x[brev(p)]
        return out
    if vec["space"] == "fwd_half":
        w2i = pow(pow(7, (R - 1) >> (L + 1), R), -1, R)
        out = []
        for row in rows:
            c, p = [], 1
            for j in range(n):
                c.append(row[j] * p % R)
                p = p * w2i % R
            ninv = pow(n, -1, R)
            out.append([v * ninv % R for v in dft_fast(c, L)])
        return out
    return rows


def _block_inverse(seg, TA, inverse):
    """positions-in, positions-out inverse of `TA` DIT stages on one block: the block's input positions hold
    brev-ordered data, so this returns a[] values (DIT position order on entry) whose first pass leaves `seg`"""
    m = 1 << TA
    # natural-order data whose m-point transform (unscaled, with the pass's root) is seg
    nat = dft_fast(seg, TA, inverse=not inverse)
    if inverse:
        nat = [v * pow(m, -1, R) % R for v in nat]
    return [nat[brev(i, TA)] for i in range(m)]


def run_vector(vec):
    """-> (reached value per target, largest value anywhere, outputs per transform)"""
    rows = materialise(vec)
    L = vec["logn"]
    res = [das(r, L) if vec["shape"] == "das" else transform(r, L, vec["shape"] == "inv") for r in rows]
    reached = [res[b]["reached"][p][o] for b, p, o in vec["targets"]]
    return reached, max(r["top"] for r in res), [r["out"] for r in res]


def _vec(name, shape, L, nbatch, space, fill, seed, entries, targets, x0):
    v = dict(name=name, shape=shape, logn=L, nbatch=nbatch, space=space, fill="%x" % fill, seed=seed,
             entries=[[b, i, "%x" % val] for b, i, val in entries], targets=[list(t) for t in targets])
    reached, top, _ = run_vector(v)
    v["reached"] = ["%x" % r for r in reached]
    v["x0"] = ["%x" % x for x in x0]
    return v


def build_first_pass(name, shape, L, targets, seed=1, fill=0, x0=R - 1):
    """aimed at the first pass (the whole transform for n <= 4096): transform b aims at position targets[b]"""
    T = split_passes(L)[0]
    tw = twiddles(L, shape == "inv")
    entries = []
    for b, o in enumerate(targets):
        chosen = aim_pass(o, 0, T, tw, True, x0 - b, fill, seed + b)  # a different start and seed per transform
        entries += [(b, brev(p, L), v) for p, v in sorted(chosen.items())]
    return _vec(name, shape, L, len(targets), "input", fill, seed, entries, [(b, 0, o) for b, o in enumerate(targets)],
                [x0 - b for b in range(len(targets))])


def build_second_pass(name, shape, L, o, seed=1, x0=R - 1):
    """aimed at the kind-B pass of a two-pass transform: the entries are the residues between the passes"""
    TA, TB = split_passes(L)
    chosen = aim_pass(o, TA, TB, twiddles(L, shape == "inv"), False, x0, 0, seed)
    return _vec(name, shape, L, 1, "boundary", 0, seed, [(0, p, v) for p, v in sorted(chosen.items())], [(0, 1, o)], [x0])


def build_das(name, L, o, seed=1):
    """the forward half of the fused DAS extension aimed at o.  The forward half reads t + r, t = mul_signed(lazy
    inverse result, twist) congruent to the chosen residue: residue + r or residue, which is known only once the evens
    are; a few rounds of choosing, transforming back and running the inverse half settle it."""
    n = 1 << L
    tw = twiddles(L, False)
    off, x0res, y0res, best = {}, 0, 0, None
    for _ in range(8):
        def lazy_of(p, v, off=off):
            return v + (R if v == 0 else off.get(brev(p, L), 0))
        chosen = aim_pass(o, 0, L, tw, True, x0res, 0, seed, lazy_of)
        chosen[0] = x0res
        if o & 1:
            chosen[1] = y0res  # stage 0 subtracts this input as it is: the smallest lazy value the twist can leave
        entries = [(0, brev(p, L), v) for p, v in sorted(chosen.items())]
        v = dict(name=name, shape="das", logn=L, nbatch=1, space="fwd_half", fill="0", seed=seed,
                 entries=[[b, i, "%x" % val] for b, i, val in entries], targets=[[0, 1, o]])
        res = das(materialise(v)[0], L)
        reached = res["reached"][1][o]
        if best is None or reached > best[0]:
            v["reached"] = ["%x" % reached]
            v["x0"] = ["%x" % res["fwd_in"][0]]
            best = (reached, v)
        # what the twist really added to each chosen residue, and the residues at positions 0 and n / 2 that sit
        # an eighth below / above the edge a W / 2^261 of their twist (positive t: residue + r; negative: residue)
        off = {j: res["fwd_in"][j] - val for _, j, val in entries}
        edge0 = res["reached"][0][0] * ONE >> K
        x0res = edge0 - (edge0 >> 3)
        edge1 = res["reached"][0][n >> 1] * (ONE * pow(7, ((R - 1) >> (L + 1)) * (n >> 1), R) % R) >> K
        y0res = edge1 + (edge1 >> 3) + 1
    return best[1]


def tile_targets(L, count):
    """a different output in neighbouring transforms of a tile: 2^L - 1 and 2^L - 2, the two outputs whose chains take
    the +5r (+4r, +8r) branch at every stage above the first — every other output stays a whole 3r per cleared bit
    below, no further from what random inputs reach than from the bound"""
    return [(1 << L) - 1 - (b & 1) for b in range(count)]


def build_all():
    top = (1 << 256) - 1
    v = []
    for shape in ("fwd", "inv"):
        v.append(build_first_pass(shape + "4096_last", shape, 12, [4095]))
        v.append(build_first_pass(shape + "4096_seed2", shape, 12, [4095], seed=2, x0=R - 2))
        v.append(build_first_pass(shape + "4096_bf1n", shape, 12, [4094]))
    v.append(build_first_pass("fwd512_tile", "fwd", 9, tile_targets(9, 8)))
    v.append(build_first_pass("inv512_tile", "inv", 9, tile_targets(9, 8), seed=5))
    v.append(build_first_pass("fwd64_tile", "fwd", 6, tile_targets(6, 64)))
    for L in (13, 14):
        TA = split_passes(L)[0]
        v.append(build_first_pass("fwd2p%d_first_pass" % L, "fwd", L, [(5 << TA) + (1 << TA) - 1]))
        v.append(build_second_pass("fwd2p%d_second_pass" % L, "fwd", L, (1 << L) - 1))
    v.append(build_second_pass("inv2p14_second_pass", "inv", 14, (1 << 14) - 1, seed=3))
    v.append(build_das("das4096", 12, 4095))
    v.append(build_das("das256", 8, 255))
    v.append(build_first_pass("fwd4096_fill_r_minus_1", "fwd", 12, [4095], fill=R - 1))
    v.append(build_first_pass("fwd4096_fill_2p256_minus_1", "fwd", 12, [4095], fill=top, x0=top))
    return v
