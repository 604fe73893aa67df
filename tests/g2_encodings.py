"""A catalogue of 96-byte compressed G2 encodings with the answer every decoder and subgroup test of the library must
give, in the manner of tests/g1_encodings.py and derived with tests/codec_model.py alone (Python integers).

catalogue() -> [(name, bytes96, cls)], cls 0 = a valid element (a point of G2, or infinity), 1 = no encoding of a point
of the twist, 2 = a point of E'(Fp2): y^2 = x^3 + 4(1 + u) outside the prime-order subgroup G2.  Every cls comes out of
codec_model.classify(): the flag rules, both halves of x below p, the norm criterion for a square of Fp2, and [r]P == O.

The outside points: #E'(Fp2) = r * H2 with H2 = 13^2 * 23^2 * 2713 * 11953 * 262069 * (a large cofactor); the model finds
the small primes by trial division and a torsion point T for each.  Points of full order (small x) and sums T + Q with Q
in G2 are there as well: for the latter psi(P) - [x]P is the same as for T alone."""
import functools
import random

import codec_model as M

P = M.P
FLAG_MASK = (1 << 381) - 1


def payload(b):
    return int.from_bytes(b[:48], "big") & FLAG_MASK, int.from_bytes(b[48:], "big")


@functools.lru_cache(maxsize=None)
def catalogue():
    M.self_check()
    rnd = random.Random(762)
    out = []

    def put(name, b, want=None):
        cls = M.classify(b)
        assert want is None or cls == want, (name, b.hex(), cls, want)
        out.append((name, b, cls))

    # -- valid
    put("infinity", M.compress(None), 0)
    ks = [1, 2, 3, M.R - 1, M.R - 2] + [rnd.randrange(1, M.R) for _ in range(11)]
    pts = []
    for k in ks:
        a = M.mul(k, M.G2)
        pts.append(a)
        tag = str(k) if k < 4 else "(r-%d)" % (M.R - k) if M.R - k < 4 else hex(k)[:10] + ".."
        put("%sG" % tag, M.compress(a), 0)
        if k > 3 and M.R - k > 3:
            put("-%sG" % tag, M.compress(M.neg(a)), 0)  # both signs of a valid point
    for b in M.golden_g2_bytes()[1:4]:
        put("setup point " + b.hex()[:8], b, 0)
    signs = [b[0] >> 5 & 1 for _, b, c in out if c == 0 and not b[0] & 0x40]
    assert signs.count(0) >= 8 and signs.count(1) >= 8, signs

    # -- on the twist, outside G2
    primes = M.small_cofactor_primes()
    assert primes[0] == 13 and len(primes) >= 4, primes
    for q in primes:
        t = M.torsion_point(q)
        put("order %d" % q, M.compress(t), 2)
        put("order %d, negated" % q, M.compress(M.neg(t)), 2)
        put("order %d + G" % q, M.compress(M.add(t, M.G2)), 2)
        put("order %d + a multiple of G" % q, M.compress(M.add(t, pts[7])), 2)
    c0, found = 0, 0
    while found < 4:  # the smallest real x on the twist, both signs: points of (nearly) full order
        c0 += 1
        a = M.point_with_x((c0, 0), 0)
        if a is not None:
            assert M.mul(M.H2, a) is not None and M.mul(M.R, a) is not None
            put("x = %d, sign 0" % c0, M.raw(4, 0, c0), 2)
            put("x = %d, sign 1" % c0, M.raw(5, 0, c0), 2)
            found += 1
    for c1 in (1, 2, 3, 4, 5, 6):  # and purely imaginary x
        if M.point_with_x((0, c1), 0) is not None:
            put("x = %d u, sign 0" % c1, M.raw(4, c1, 0), 2)
            put("x = %d u, sign 1" % c1, M.raw(5, c1, 0), 2)

    # -- flags
    valid = [b for _, b, c in out if c == 0 and not b[0] & 0x40]
    v0 = next(b for b in valid if not b[0] & 0x20)
    v1 = next(b for b in valid if b[0] & 0x20)
    for top3 in range(8):
        for what, (c1, c0) in (("zero", (0, 0)), ("x of a sign-0 point", payload(v0)), ("x of a sign-1 point", payload(v1))):
            put("flags %s over %s" % (format(top3, "03b"), what), M.raw(top3, c1, c0))
    put("infinity with the sign flag", M.raw(7, 0, 0), 1)
    put("infinity, a bit in the first half", b"\xc0" + bytes(22) + b"\x10" + bytes(72), 1)
    put("infinity, the last bit of the first half", b"\xc0" + bytes(46) + b"\x01" + bytes(48), 1)
    put("infinity, the first bit of the second half", b"\xc0" + bytes(47) + b"\x80" + bytes(47), 1)
    put("infinity, the last bit of the second half", b"\xc0" + bytes(94) + b"\x01", 1)
    put("compression flag missing", bytes([valid[3][0] & 0x7F]) + valid[3][1:], 1)

    # -- range: either half of x at p, p - 1, 2^381 - 1 (2^384 - 1 for the half without flags)
    gc1, gc0 = payload(v0)
    put("x.c1 = p", M.raw(4, P, gc0), 1)
    put("x.c0 = p", M.raw(4, gc1, P), 1)
    put("x.c1 = p, x.c0 = 0", M.raw(4, P, 0), 1)
    put("x.c1 = 0, x.c0 = p", M.raw(4, 0, P), 1)
    put("x.c1 = 2^381 - 1", M.raw(4, (1 << 381) - 1, gc0), 1)
    put("x.c0 = 2^381 - 1", M.raw(4, gc1, (1 << 381) - 1), 1)
    put("x.c0 = 2^384 - 1", M.raw(4, gc1, (1 << 384) - 1), 1)
    put("x.c0 = p + 1", M.raw(4, 0, P + 1), 1)
    for sign in (0, 1):
        put("x.c1 = p - 1, sign %d" % sign, M.raw(4 | sign, P - 1, gc0))
        put("x.c0 = p - 1, sign %d" % sign, M.raw(4 | sign, gc1, P - 1))
        put("x = (p - 1)(1 + u), sign %d" % sign, M.raw(4 | sign, P - 1, P - 1))

    # -- x^3 + b' is not a square
    c0, found = 0, 0
    while found < 3:
        c0 += 1
        if M.point_with_x((c0, 0), 0) is None:
            put("x = %d: x^3 + b' is not a square" % c0, M.raw(4, 0, c0), 1)
            found += 1
    c1, found = 0, 0
    while found < 2:
        c1 += 1
        if M.point_with_x((7, c1), 0) is None:
            put("x = 7 + %d u: x^3 + b' is not a square" % c1, M.raw(5, c1, 7), 1)
            found += 1
    assert len({name for name, _, _ in out}) == len(out)
    assert all(sum(1 for _, _, c in out if c == k) >= 20 for k in (0, 1, 2))
    return tuple(out)


def by_class(cls):
    return [(name, b) for name, b, c in catalogue() if c == cls]
