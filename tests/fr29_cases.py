"""Cases and checkers for the Fr arithmetic of the NTT kernels (fr29.hip.h) and the lane scan of frscan.hip.h, against
Python integers.  Shared by the host test (tests/test_host_cpu.py, the header compiled with the host compiler), the
CPU module tests/test_fr_device_cases_cpu.py and the GPU module tests/test_fr_arith_gpu.py (tests/device_checks/
fr_check.hip, the same header compiled for the device).

A case is (op, operands, checker): operands are lists of u32 words (an Fe is 9 limbs of 29 bits, the top limb signed; an
Fr is 8 words of 32 bits), the checker takes the list of output words and raises AssertionError.  The wire format is one
line per case, `op` followed by the operand words in hex; a harness answers one line of hex words per case.

base_cases() is the case set the host test has always run (same seed, same order); new_cases() adds mul_signed2, the
first round of a transform, the DAS twist, the bit re-slicing and mul_blst; scan_cases() is device-only."""
import random

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
M29 = (1 << 29) - 1
RINV = pow(1 << 261, -1, R)      # the 29-bit multipliers divide by 2^261
RINV256 = pow(1 << 256, -1, R)   # mul_blst divides by 2^256
TOP = 0x73eda7                   # r >> 232

# words in, words out per op (the harness holds the same table)
SHAPES = {"round": (72, 36), "msig": (18, 9), "bfs": (18, 18), "bfl": (18, 18), "bfl8": (18, 18), "redl": (9, 8),
          "fin": (18, 8), "mul": (18, 9), "msig2": (36, 18), "round_unit": (41, 36), "twist": (18, 9), "pack": (9, 8),
          "unpack": (8, 9), "unpack_shl5": (8, 9), "mulb": (16, 8), "scan": (64 * 8 + 1 + 6 * 8, 64 * 8)}
HOST_OPS = ("round", "msig", "bfs", "bfl", "bfl8", "redl", "fin", "mul")
NEW_OPS = ("msig2", "round_unit", "twist", "pack", "unpack", "unpack_shl5", "mulb")


def limbs(v):
    assert 0 <= v < 1 << (232 + 31)
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def sval(l):  # top limb signed
    top = l[8] - (1 << 32) if l[8] >> 31 else l[8]
    return sum(x << (29 * i) for i, x in enumerate(l[:8])) + (top << 232)


def words(v):
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def wval(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


def normalized(l):
    return all(x <= M29 for x in l[:8]) and not l[8] >> 31


def _fail(msg):
    raise AssertionError(msg)


def base_cases():
    rnd = random.Random(2929)

    def edge(k):
        out = [0, 1, k * R - 1, (1 << 232) - 1, 1 << 232]
        for j in range(0, k, max(1, k // 8)):
            out += [j * R, j * R + 1, max(0, j * R - 1)]
        return [v for v in out if v < k * R] + [rnd.randrange(k * R) for _ in range(30)]

    cases = []

    # ---- one radix-4 round, the way ntt_round<..., FIRST = false> runs it: inputs normalised, value < 51r ----
    def chk_round(es, ws):
        def net(e, w):
            e = list(e)
            for (a, b, wi) in ((0, 1, 0), (2, 3, 1), (0, 2, 2), (1, 3, 3)):
                t = e[b] * w[wi] * RINV
                e[a], e[b] = e[a] + t, e[a] - t
            return e

        want = net(es, ws)

        def chk(out):
            got = [out[9 * i:9 * i + 9] for i in range(4)]
            for g, w, e in zip(got, want, es):
                assert normalized(g), "round output not normalised"
                assert (sval(g) - w) % R == 0, "round residue"
                assert 0 <= sval(g) < max(es) + 10 * R + 1, "round growth"
        return chk

    for _ in range(400):
        top = rnd.choice([1, 2, 8, 30, 51])
        es = [rnd.choice(edge(top)) for _ in range(4)]
        ws = [rnd.choice([0, 1, R - 1, rnd.randrange(R), rnd.randrange(R)]) for _ in range(4)]
        cases.append(("round", [limbs(e) for e in es] + [limbs(w) for w in ws], chk_round(es, ws)))
    # ---- mul_signed alone on lazy multiplicands: limbs up to 1.5 * 2^30, top limb down to -1 ----
    for _ in range(400):
        a = [rnd.randrange(3 << 29) for _ in range(8)] + [rnd.choice([0, 1, 0xFFFFFFFF, rnd.randrange(64 * 0x73eda7)])]
        if not -R < sval(a) < 64 * R:
            continue
        b = rnd.choice([0, 1, R - 1, rnd.randrange(R)])
        cases.append(("msig", [a, limbs(b)], chk_msig(sval(a) * b)))
    # ---- the three butterflies: values and limb growth ----
    for _ in range(300):
        x = rnd.choice(edge(51))
        t = rnd.randrange(-R + 1, 2 * R)  # what mul_signed returns, or a normalised value below 2r
        tl = [(t >> (29 * i)) & M29 for i in range(8)] + [(t >> 232) & 0xFFFFFFFF]

        def chk_s(out, x=x, t=t):
            a, b = out[:9], out[9:]
            assert sval(a) == x + t + R and sval(b) == x + 4 * R - t
            assert all(v < (1 << 29) + (1 << 30) for v in a[:8] + b[:8])
        cases.append(("bfs", [limbs(x), tl], chk_s))
        t3 = rnd.choice(edge(3))
        cases.append(("bfl", [limbs(x), limbs(t3)], lambda out, x=x, t=t3: (sval(out[:9]) == x + t and sval(out[9:]) == x + 4 * R - t and all(v < 3 << 29 for v in out[:8] + out[9:17])) or _fail("bfl")))
        t7 = rnd.choice(edge(7))
        cases.append(("bfl8", [limbs(x), limbs(t7)], lambda out, x=x, t=t7: (sval(out[:9]) == x + t and sval(out[9:]) == x + 8 * R - t and all(v < 3 << 29 for v in out[:8] + out[9:17])) or _fail("bfl8")))
    # ---- reduce_lazy / finish: every multiple of r below 64r with its neighbours, the maximum, random ----
    vals = [64 * R - 1]
    for j in range(64):
        vals += [j * R, j * R + 1, j * R + R - 1, j * R + (R >> 1)]
    vals += [rnd.randrange(64 * R) for _ in range(3000)]
    for v in vals:
        cases.append(("redl", [limbs(v)], lambda out, v=v: wval(out) == v % R or _fail("reduce_lazy %x" % v)))
    for v in vals[:600]:
        m = rnd.choice([1, R - 1, rnd.randrange(R)])
        cases.append(("fin", [limbs(v), limbs(m)], lambda out, v=v, m=m: wval(out) == v * m * RINV % R or _fail("finish")))
    # ---- mul: multiplicand limbs < 2^31, multiplier normalised, a*b < 2^261 r ----
    for _ in range(300):
        a = [rnd.randrange(1 << 31) for _ in range(8)] + [rnd.randrange(64 * 0x73eda7)]
        b = rnd.randrange(R)
        if sval(a) * b < (R << 261):
            cases.append(("mul", [a, limbs(b)], lambda out, w=sval(a) * b: (normalized(out) and sval(out) < 2 * R and (sval(out) - w * RINV) % R == 0) or _fail("mul")))
    return cases


def chk_msig(want):
    """mul_signed: limbs 0..7 normalised, value in (-r, r), congruent to want * 2^-261"""
    def chk(out):
        assert all(x <= M29 for x in out[:8]) and -R < sval(out) < R and (sval(out) - want * RINV) % R == 0
    return chk


def _lazy_operand(rnd):
    """a multiplicand as a butterfly leaves it: limbs up to 1.5 * 2^30, top limb down to -1, value in (-r, 64r)"""
    while True:
        a = [rnd.randrange(3 << 29) for _ in range(8)] + [rnd.choice([0, 1, 0xFFFFFFFF, rnd.randrange(64 * TOP)])]
        if -R < sval(a) < 64 * R:
            return a


def _edge_pairs(rnd):
    """(multiplicand limbs, canonical multiplier): the corners of mul_signed's domain"""
    big = [3 * (1 << 29) - 1] * 8  # every low limb at its maximum
    top_for_64r = (64 * R - 1 - sval(big + [0])) >> 232
    out = [(limbs(0), 0), (limbs(0), R - 1), (limbs(64 * R - 1), R - 1), (limbs(64 * R - 1), 1),
           (big + [top_for_64r], R - 1), (big + [0xFFFFFFFF], R - 1), ([0] * 8 + [0xFFFFFFFF], R - 1),
           ([M29] * 8 + [0xFFFFFFFF], 1), (limbs(63 * R), (1 << 254) + 1), (limbs(R), R - 1)]
    # a product that is a small residue: the result lies just above -r (the case the transforms' worst inputs aim at)
    for k in (1, 2, 57, 63):
        b = rnd.randrange(1, R)
        lo = (k * R * b >> 261) + 1  # the residue just above a*b / 2^261
        a = k * R + (lo * pow(b, -1, R) << 261) % R
        out.append((limbs(a), b))
    return [(a, b) for a, b in out if -R < sval(a) < 64 * R]


def new_cases():
    rnd = random.Random(2930)
    cases = []
    cross = []  # (index of a msig2 case, indices of the msig cases of its two pairs), indices into `cases`
    edges = _edge_pairs(rnd)
    # ---- mul_signed2: an edge pair next to an ordinary one, both orders; every pair also alone through mul_signed ----
    pairs = []
    for i in range(120):
        e = edges[i % len(edges)] if i % 3 != 2 else (_lazy_operand(rnd), rnd.choice([0, 1, R - 1, rnd.randrange(R)]))
        o = (_lazy_operand(rnd), rnd.randrange(R))
        pairs.append((e, o) if i & 1 else (o, e))
    for _ in range(40):  # two independent edge pairs
        pairs.append((rnd.choice(edges), rnd.choice(edges)))
    singles = []
    for (a0, b0), (a1, b1) in pairs:
        def chk2(out, w0=sval(a0) * b0, w1=sval(a1) * b1):
            chk_msig(w0)(out[:9])
            chk_msig(w1)(out[9:])
        cases.append(("msig2", [a0, limbs(b0), a1, limbs(b1)], chk2))
        singles.append((len(cases) - 1, (a0, b0), (a1, b1)))
    for i2, p0, p1 in singles:
        idx = []
        for a, b in (p0, p1):
            cases.append(("msig", [a, limbs(b)], chk_msig(sval(a) * b)))
            idx.append(len(cases) - 1)
        cross.append((i2, idx[0], idx[1]))

    # ---- the first round of a transform: KZG_BF1 x 2, KZG_BF1N(0, 2), KZG_BF(1, 3, w), one norm ----
    def chk_unit(xs, w):
        a, b, c, d = xs
        e0, e1, e2, e3 = a + b, a + 4 * R - b, c + d, c + 4 * R - d
        want = [e0 + e2, None, e0 + 8 * R - e2, None]  # exact values; elements 1 and 3 by residue
        res13 = [(e1 + e3 * w * RINV) % R, (e1 - e3 * w * RINV) % R]

        def chk(out):
            got = [out[9 * i:9 * i + 9] for i in range(4)]
            for g in got:
                assert normalized(g), "first round output not normalised"
                assert 0 <= sval(g) < max(xs) + 13 * R, "first round growth"
            assert sval(got[0]) == want[0] and sval(got[2]) == want[2], "first round, multiplication-free pair"
            assert sval(got[1]) % R == res13[0] and sval(got[3]) % R == res13[1], "first round residue"
            assert sval(got[1]) + sval(got[3]) == 2 * e1 + 5 * R, "first round pair sum"
        return chk

    tops = [0, 1, R - 1, R, (1 << 255) - 1, 1 << 255, (1 << 256) - 1, (1 << 256) - 2, 2 * R, 2 * R + 1]
    for i in range(300):
        if i < 100:
            xs = [rnd.choice([0, 1, R - 1, rnd.randrange(R)]) for _ in range(4)]
        else:
            xs = [rnd.choice(tops + [rnd.randrange(1 << 256)] * 4) for _ in range(4)]
        if i in (0, 100):
            xs = [R - 1] * 4 if i == 0 else [(1 << 256) - 1] * 4
        if i in (2, 102):
            xs = [xs[0], 0, 0, 0] if i == 2 else [(1 << 256) - 1, 0, (1 << 256) - 1, 0]
        w = rnd.choice([1, R - 1, rnd.randrange(R), rnd.randrange(R)])
        cases.append(("round_unit", [words(x) for x in xs] + [limbs(w)], chk_unit(xs, w)))

    # ---- the DAS twist: mul_signed by a canonical multiplier, + r, norm ----
    for i in range(200):
        a, b = edges[i % len(edges)] if i % 2 == 0 else (_lazy_operand(rnd), rnd.choice([0, 1, R - 1, rnd.randrange(R)]))
        if not normalized(a) or sval(a) < 0:  # the twist follows a round's norm
            a = limbs(rnd.choice([0, 1, R - 1, 63 * R + 5, 64 * R - 1, rnd.randrange(64 * R)]))

        def chk_t(out, want=sval(a) * b):
            assert normalized(out) and 0 < sval(out) < 2 * R and (sval(out) - want * RINV) % R == 0
        cases.append(("twist", [a, limbs(b)], chk_t))

    # ---- bit re-slicing ----
    vals = [0, 1, R - 1, R, (1 << 256) - 1, (1 << 255), M29, 1 << 29, (1 << 232) - 1, 1 << 232, 0x5555 * ((1 << 256) // 0xFFFF),
            0xAAAA * ((1 << 256) // 0xFFFF)] + [(1 << k) - 1 for k in range(28, 256, 29)] + [1 << k for k in range(0, 256, 31)]
    vals += [rnd.randrange(1 << 256) for _ in range(100)]
    for v in vals:
        cases.append(("pack", [limbs(v)], lambda out, v=v: wval(out) == v or _fail("pack %x" % v)))
        cases.append(("unpack", [words(v)], lambda out, v=v: (normalized(out) and out == limbs(v)) or _fail("unpack %x" % v)))
        cases.append(("unpack_shl5", [words(v)], lambda out, v=v: (normalized(out) and sval(out) == 32 * v and all(x <= M29 for x in out)) or _fail("unpack_shl5 %x" % v)))

    # ---- mul_blst: a * b * 2^-256 mod r in [0, r), operands below 2^256 with a * b < 2^256 * r ----
    ab = []
    small = [0, 1, R - 1, rnd.randrange(R), rnd.randrange(R)]
    for a in (0, 1, R - 1, (1 << 256) - 1):
        for b in small:
            ab += [(a, b), (b, a)]
    for a in ((1 << 256) - 1, (1 << 256) - 2, R, R + 1, 1 << 255, rnd.randrange(R, 1 << 256), rnd.randrange(R, 1 << 256)):
        b = min(((R << 256) - 1) // a, (1 << 256) - 1)  # the largest partner
        ab += [(a, b), (b, a), (a, b - 1)]
    ab += [(rnd.randrange(R), rnd.randrange(R)) for _ in range(150)]
    for a, b in ab:
        assert a * b < R << 256
        cases.append(("mulb", [words(a), words(b)], lambda out, w=a * b: wval(out) == w * RINV256 % R or _fail("mul_blst")))
    return cases, cross


def all_cases():
    """base_cases() + new_cases() as one list, with the cross-check indices of the mul_signed2 cases into it"""
    base = base_cases()
    new, cross = new_cases()
    return base + new, [tuple(i + len(base) for i in c) for c in cross]


def scan_model(S, gw, C):
    """what scan_suffix returns in the lanes of a wave: S, C in Montgomery form (x * 2^256 mod r)"""
    out = []
    for lane in range(64):
        lg, base = lane % gw, lane - lane % gw
        acc, p = 0, 1 << 256  # C^d in Montgomery form
        for d in range(gw - lg):
            acc += p * S[base + lg + d] * RINV256
            p = p * C * RINV256 % R
        out.append(acc % R)
    return out


def scan_cases():
    """scan_suffix for every group width, a different C per case; a case is one wave: 64 lanes' S, gw, C^(2^k), k < 6"""
    rnd = random.Random(2931)
    cases = []
    for gw in (1, 2, 4, 8, 16, 32, 64):
        for style in range(4):
            C = R - 1 if (gw, style) == (64, 2) else rnd.randrange(2, R)  # a different C per case
            S = []
            for lane in range(64):
                pick = (style + lane // max(1, gw // 2) + lane) % 4 if style < 3 else 3
                S.append([0, R - 1, rnd.randrange(R), rnd.randrange(R)][pick])
            if style == 1:  # idle lanes: whole groups and the tail of a group carry zeros
                S = [0 if (lane // gw) % 3 == 2 or lane % gw >= max(1, gw - gw // 4) else s for lane, s in enumerate(S)]
            if style == 2:
                S = [R - 1] * 64
            pw, p = [], C
            for _ in range(6):
                pw.append(p)
                p = p * p * RINV256 % R
            want = scan_model(S, gw, C)

            def chk(out, want=want):
                got = [wval(out[8 * i:8 * i + 8]) for i in range(64)]
                bad = [i for i in range(64) if got[i] != want[i]]
                assert not bad, "scan_suffix lanes %s" % bad[:8]
            cases.append(("scan", [sum((words(s) for s in S), []), [gw], sum((words(p) for p in pw), [])], chk))
    return cases


def encode(cases):
    text = []
    for op, ops, _ in cases:
        flat = [x for l in ops for x in l]
        assert len(flat) == SHAPES[op][0], (op, len(flat))
        text.append(op + " " + " ".join("%x" % x for x in flat) + "\n")
    return "".join(text)


def failures(cases, text, cross=()):
    """-> [(op, index of the case among the cases of its op, message)]"""
    lines = text.strip().split("\n")
    if len(lines) != len(cases):
        return [("*", -1, "%d output lines for %d cases" % (len(lines), len(cases)))]
    nth, seen, outs, bad = [], {}, [], []
    for op, _, _ in cases:
        nth.append(seen.get(op, 0))
        seen[op] = nth[-1] + 1
    for i, ((op, ops, chk), ln) in enumerate(zip(cases, lines)):
        got = None
        try:
            got = [int(x, 16) for x in ln.split()]
            assert len(got) == SHAPES[op][1], "%d output words" % len(got)
            chk(got)
        except (AssertionError, ValueError) as e:
            bad.append((op, nth[i], "%s -> %s: %s" % ([hex(sval(l)) if len(l) == 9 else l[:8] for l in ops][:8], ln[:400], e)))
        outs.append(got if got is not None and len(got) == SHAPES[op][1] else None)
    flagged = {(op, k) for op, k, _ in bad}
    for i2, ia, ib in cross:  # mul_signed2 against mul_signed on the same pairs: limb for limb; a difference is charged
        # to the mul_signed2 case unless the lone case already failed its own checker
        if outs[i2] is None or outs[ia] is None or outs[ib] is None:
            continue
        for half, i1 in ((0, ia), (1, ib)):
            if outs[i2][9 * half:9 * half + 9] != outs[i1] and (cases[i1][0], nth[i1]) not in flagged and (cases[i2][0], nth[i2]) not in flagged:
                bad.append((cases[i2][0], nth[i2], "mul_signed2 result %d differs from mul_signed on the same operands" % half))
    return bad
