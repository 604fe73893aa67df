"""A catalogue of 48-byte compressed G1 encodings with the answer every decoder and subgroup test of the library must
give, derived here with Python integers alone: no oracle, no library, nothing from the code under test.

catalogue() -> [(name, bytes48, cls)], cls 0 = a valid element (a point of G1, or infinity), 1 = no encoding of a curve
point, 2 = a point of the curve y^2 = x^3 + 4 over F_p that lies outside the prime-order subgroup G1.  Every cls comes
out of classify(): the flag rules of the ZCash format, x < p, the Euler criterion and [r]P == O.

What makes the outside points interesting: #E(F_p) = h * r with the cofactor h = 3 * 11^2 * 10177^2 * 859267^2 *
52437899^2, and the BLS parameter is 1 modulo each of those primes, so for a torsion point T of order q | h:
[|x|]T = -T and [x^2]T = T.  The endomorphism test phi(P) == -[x^2]P of the library then has to tell phi(T) from -T, and
for q = 3 (the points (0, +-2)) its double-and-add chain passes through infinity on the way."""
import functools
import random

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
BLS_X = 0xd201000000010000  # |x|; the parameter itself is negative
COFACTOR_PRIMES = (3, 11, 10177, 859267, 52437899)
H = 3 * (11 * 10177 * 859267 * 52437899) ** 2
G = (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
     0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1)
assert H == (BLS_X + 1) ** 2 // 3 and all((-BLS_X) % q == 1 for q in COFACTOR_PRIMES)


# ---- the curve, affine, None = the point at infinity
def add(a, b):
    if a is None or b is None:
        return b if a is None else a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def neg(a):
    return None if a is None else (a[0], -a[1] % P)


def mul(k, a):
    acc = None
    for bit in bin(k)[2:]:
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, a)
    return acc


def on_curve(a):
    return a is None or (a[1] * a[1] - a[0] ** 3 - 4) % P == 0


# ---- the encoding
def compress(a):
    if a is None:
        return b"\xc0" + bytes(47)
    x, y = a
    return (x | 1 << 383 | (y > (P - 1) // 2) << 381).to_bytes(48, "big")


def raw(top3, x):
    """the three flag bits over a 381-bit payload, whatever they mean"""
    assert 0 <= top3 < 8 and 0 <= x < 1 << 381
    return (top3 << 381 | x).to_bytes(48, "big")


def decode(b):
    """the point a valid encoding names (None for infinity); raises ValueError for what is no encoding of a curve point"""
    assert len(b) == 48
    compressed, infinity, sort = b[0] >> 7 & 1, b[0] >> 6 & 1, b[0] >> 5 & 1
    x = int.from_bytes(b, "big") & ((1 << 381) - 1)
    if not compressed:
        raise ValueError("compression flag missing")
    if infinity:
        if sort or x:
            raise ValueError("infinity with further bits set")
        return None
    if x >= P:
        raise ValueError("x >= p")
    rhs = (x * x * x + 4) % P
    if rhs and pow(rhs, (P - 1) // 2, P) != 1:  # Euler: no y with y^2 = x^3 + 4
        raise ValueError("x^3 + 4 is not a square")
    y = pow(rhs, (P + 1) // 4, P)  # p = 3 (mod 4)
    assert y * y % P == rhs
    if (y > (P - 1) // 2) != bool(sort):
        y = -y % P
    return x, y


def classify(b):
    try:
        a = decode(b)
    except ValueError:
        return 1
    return 0 if mul(R, a) is None else 2


def point_with_x(x, sign):
    """the curve point with this x whose y has the given sign flag, or None if x^3 + 4 is not a square"""
    try:
        return decode(raw(4 | sign, x))
    except ValueError:
        return None


def torsion_point(q):
    """a point of exact prime order q | h: the cofactor (and r) cleared from the first curve point with small x that
    leaves something"""
    full = H * R
    while full % q == 0:
        full //= q
    for x in range(1, 6):
        a = point_with_x(x, 0)
        if a is None:
            continue
        t = mul(full, a)  # order a power of q
        while t is not None and mul(q, t) is not None:
            t = mul(q, t)
        if t is not None:
            assert on_curve(t) and mul(q, t) is None
            return t
    raise AssertionError("no point of order %d from x <= 5" % q)


@functools.lru_cache(maxsize=None)
def catalogue():
    rnd = random.Random(381)
    out = []

    def put(name, b, want=None):
        cls = classify(b)
        assert want is None or cls == want, (name, b.hex(), cls, want)
        out.append((name, b, cls))

    # -- valid
    put("infinity", compress(None), 0)
    ks = [1, 2, 3, R - 1, R - 2] + [rnd.randrange(1, R) for _ in range(24)]
    for k in ks:
        put("%sG" % (k if k < 4 else "(r-%d)" % (R - k) if R - k < 4 else hex(k)[:10] + ".."), compress(mul(k, G)), 0)
    k0, step = rnd.randrange(1, R), rnd.randrange(1, R)
    cur, d, multiples = mul(k0, G), mul(step, G), []
    for _ in range(2000):  # the multiples k0 + i * step of G
        multiples.append(cur)
        cur = add(cur, d)
    put("smallest x of 2000 multiples", compress(min(multiples)), 0)
    put("largest x of 2000 multiples", compress(max(multiples)), 0)
    signs = [b[0] >> 5 & 1 for _, b, c in out if c == 0 and not b[0] & 0x40]
    assert signs.count(0) >= 8 and signs.count(1) >= 8, signs

    # -- on the curve, outside G1
    put("(0, 2)", compress((0, 2)), 2)
    put("(0, -2)", compress((0, P - 2)), 2)
    assert mul(3, (0, 2)) is None
    orders = []
    for q in COFACTOR_PRIMES:
        t = torsion_point(q)
        assert t is not None and mul(q, t) is None
        orders.append(q)
        put("order %d" % q, compress(t), 2)
        put("order %d, negated" % q, compress(neg(t)), 2)
        put("order %d + G" % q, compress(add(t, G)), 2)
    x, found = 0, 0
    while found < 6:  # the smallest x >= 1 on the curve, both signs
        x += 1
        if point_with_x(x, 0) is not None:
            put("x = %d, sign 0" % x, raw(4, x), 2)
            put("x = %d, sign 1" % x, raw(5, x), 2)
            found += 1
    assert len(orders) == 5 and sum(1 for _, _, c in out if c == 2) >= 27

    # -- flags and range
    valid = [b for _, b, c in out if c == 0 and not b[0] & 0x40]
    v0 = next(b for b in valid if not b[0] & 0x20)
    v1 = next(b for b in valid if b[0] & 0x20)
    payloads = [("zero", 0), ("x of a sign-0 point", int.from_bytes(v0, "big") & ((1 << 381) - 1)),
                ("x of a sign-1 point", int.from_bytes(v1, "big") & ((1 << 381) - 1))]
    for top3 in range(8):
        for what, x in payloads:
            put("flags %s over %s" % (format(top3, "03b"), what), raw(top3, x))
    put("infinity, byte 0 = c1", b"\xc1" + bytes(47), 1)
    put("infinity, a bit in byte 23", b"\xc0" + bytes(22) + b"\x10" + bytes(24), 1)
    put("infinity, a bit in byte 47", b"\xc0" + bytes(46) + b"\x01", 1)
    put("x = p", raw(4, P), 1)
    put("x = p + 1", raw(4, P + 1), 1)
    put("x = 2^381 - 1", raw(4, (1 << 381) - 1), 1)
    put("x = p - 1", raw(4, P - 1))
    put("x = p - 2", raw(4, P - 2))
    x, found = 0, 0
    while found < 3:
        x += 1
        if point_with_x(x, 0) is None:
            put("x = %d: x^3 + 4 is not a square" % x, raw(4, x), 1)
            found += 1
    put("compression flag missing", bytes([valid[3][0] & 0x7F]) + valid[3][1:], 1)
    assert len({name for name, _, _ in out}) == len(out)
    return tuple(out)


def by_class(cls):
    return [(name, b) for name, b, c in catalogue() if c == cls]
