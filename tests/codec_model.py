"""G2 on Python integers: Fp2 = Fp[u]/(u^2 + 1), the twist E'(Fp2): y^2 = x^3 + 4(1 + u), its ZCash-compressed 96-byte
form, the endomorphism psi and the two membership tests.  Never imported by the product: this is what g2_io.hip.h, the
host's pairing::g2_in_g2 and the batched codec calls are held to (tests/test_point_codec_cpu.py, test_point_codec_gpu.py).

An Fp2 value is a pair (c0, c1); a point is a pair (x, y) of such pairs, None = the point at infinity.

psi = twist o Frobenius o untwist.  With w^6 = xi = 1 + u the untwist is (x, y) -> (x / w^2, y / w^3); Frobenius conjugates
the Fp2 coordinates and sends w^k to w^(k p); twisting back multiplies by w^2, w^3:
    psi(x, y) = (conj(x) / xi^((p-1)/3), conj(y) / xi^((p-1)/2)),
so the two constants are inverses of powers of 1 + u and are computed here, not copied.  psi acts on G2 as
multiplication by p = x (mod r), x the (negative) BLS parameter; psi(P) == [x]P is sufficient for P in G2 as well
(M. Scott, "A note on group membership tests for G1, G2 and GT on BLS pairing-friendly curves", ePrint 2021/1130, sec. 4).

self_check() pins the model: the generator's published compressed form, psi(G) == [x]G, the twist's group order, and
the 65 G2 points of tests/golden/trusted_setup.txt (they decode, re-encode to the same bytes and are in G2 by [r]P)."""
import functools
import os

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
BLS_X = 0xd201000000010000  # |x|; the parameter itself is negative
HALF = (P - 1) // 2
B2 = (4, 4)
G2 = ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
       0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
      (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
       0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be))
G2_COMPRESSED = bytes.fromhex(
    "93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
    "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")
_x = -BLS_X
# #E'(Fp2) = r * H2 (the order of the twist that carries G2; Budroni-Pintore, "Efficient hash maps to G2 on BLS curves")
H2 = (_x ** 8 - 4 * _x ** 7 + 5 * _x ** 6 - 4 * _x ** 4 + 6 * _x ** 3 - 4 * _x ** 2 - 4 * _x + 13) // 9


# ---- Fp2
def f2add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2neg(a):
    return (-a[0] % P, -a[1] % P)


def f2conj(a):
    return (a[0], -a[1] % P)


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2sqr(a):
    return f2mul(a, a)


def f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2mul(r, a)
        a = f2mul(a, a)
        e >>= 1
    return r


def f2_is_square(a):
    """a is a square of Fp2 iff its norm is a square of Fp (a^((p^2-1)/2) = norm(a)^((p-1)/2))"""
    n = (a[0] * a[0] + a[1] * a[1]) % P
    return n == 0 or pow(n, HALF, P) == 1


def f2sqrt(a):
    """some root of a, or None: p = 3 mod 4 (Adj, Rodriguez-Henriquez, algorithm 9)"""
    if a == (0, 0):
        return a
    a1 = f2pow(a, (P - 3) // 4)
    alpha = f2mul(f2sqr(a1), a)
    x0 = f2mul(a1, a)
    if alpha == (P - 1, 0):
        x = (-x0[1] % P, x0[0])
    else:
        x = f2mul(f2pow(f2add((1, 0), alpha), HALF), x0)
    return x if f2sqr(x) == a else None


def lex_largest(y):
    """the sign rule: the imaginary part decides, the real part when the imaginary part is zero"""
    return y[1] > HALF if y[1] else y[0] > HALF


# ---- E'(Fp2), affine
def on_curve(a):
    return a is None or f2sqr(a[1]) == f2add(f2mul(f2sqr(a[0]), a[0]), B2)


def add(a, b):
    if a is None or b is None:
        return b if a is None else a
    if a[0] == b[0]:
        if f2add(a[1], b[1]) == (0, 0):
            return None
        lam = f2mul(f2mul((3, 0), f2sqr(a[0])), f2inv(f2add(a[1], a[1])))
    else:
        lam = f2mul(f2sub(b[1], a[1]), f2inv(f2sub(b[0], a[0])))
    x3 = f2sub(f2sub(f2sqr(lam), a[0]), b[0])
    return x3, f2sub(f2mul(lam, f2sub(a[0], x3)), a[1])


def neg(a):
    return None if a is None else (a[0], f2neg(a[1]))


def mul(k, a):
    acc = None
    for bit in bin(k)[2:]:
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, a)
    return acc


# ---- the wire format: x.c1 (flags in the top three bits) | x.c0, big-endian
def compress(a):
    if a is None:
        return b"\xc0" + bytes(95)
    x, y = a
    return (x[1] | 1 << 383 | lex_largest(y) << 381).to_bytes(48, "big") + x[0].to_bytes(48, "big")


def raw(top3, c1, c0):
    """the three flag bits over two payloads, whatever they mean"""
    assert 0 <= top3 < 8 and 0 <= c1 < 1 << 381 and 0 <= c0 < 1 << 384
    return (top3 << 381 | c1).to_bytes(48, "big") + c0.to_bytes(48, "big")


def decode(b):
    """the point a valid encoding names (None for infinity); ValueError for what is no encoding of a curve point"""
    assert len(b) == 96
    compressed, infinity, sort = b[0] >> 7 & 1, b[0] >> 6 & 1, b[0] >> 5 & 1
    c1 = int.from_bytes(b[:48], "big") & ((1 << 381) - 1)
    c0 = int.from_bytes(b[48:], "big")
    if not compressed:
        raise ValueError("compression flag missing")
    if infinity:
        if sort or c1 or c0:
            raise ValueError("infinity with further bits set")
        return None
    if c1 >= P or c0 >= P:
        raise ValueError("coordinate >= p")
    x = (c0, c1)
    rhs = f2add(f2mul(f2sqr(x), x), B2)
    if not f2_is_square(rhs):
        raise ValueError("x^3 + b' is not a square")
    y = f2sqrt(rhs)
    assert y is not None and f2sqr(y) == rhs
    if lex_largest(y) != bool(sort):
        y = f2neg(y)
    return x, y


# ---- psi and membership
@functools.lru_cache(maxsize=None)
def psi_constants():
    xi = (1, 1)
    return f2inv(f2pow(xi, (P - 1) // 3)), f2inv(f2pow(xi, (P - 1) // 2))


def psi(a):
    if a is None:
        return None
    cx, cy = psi_constants()
    return f2mul(f2conj(a[0]), cx), f2mul(f2conj(a[1]), cy)


def in_g2(a):
    """the definition"""
    return mul(R, a) is None


def in_g2_psi(a):
    """psi(P) == [x]P = -[|x|]P"""
    return a is None or psi(a) == neg(mul(BLS_X, a))


def classify(b):
    """0 a point of G2 (or infinity), 1 no encoding of a curve point, 2 on the twist outside G2"""
    try:
        a = decode(b)
    except ValueError:
        return 1
    return 0 if in_g2(a) else 2


def small_cofactor_primes(limit=1 << 19):
    """the prime factors of the twist's cofactor below `limit`, by trial division"""
    out, h, q = [], H2, 2
    while q < limit:
        if h % q == 0:
            out.append(q)
            while h % q == 0:
                h //= q
        q += 1
    return out


def point_with_x(x, sign):
    try:
        return decode(raw(4 | sign, x[1], x[0]))
    except ValueError:
        return None


def torsion_point(q):
    """a point of exact prime order q | H2"""
    full = H2 * R
    while full % q == 0:
        full //= q
    for c0 in range(1, 40):
        a = point_with_x((c0, 0), 0)
        if a is None:
            continue
        t = mul(full, a)
        while t is not None and mul(q, t) is not None:
            t = mul(q, t)
        if t is not None:
            assert on_curve(t) and mul(q, t) is None
            return t
    raise AssertionError("no point of order %d" % q)


# ---- Montgomery limbs, as the headers hold constants (fp28: 14 limbs of 28 bits, radix 2^392)
def limbs28(v):
    m = v * (1 << 392) % P
    return [(m >> (28 * i)) & ((1 << 28) - 1) for i in range(14)]


def golden_g2_bytes():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trusted_setup.txt")
    tok = open(path).read().split()
    n1, n2 = int(tok[0]), int(tok[1])
    return [bytes.fromhex(t) for t in tok[2 + n1:2 + n1 + n2]]


@functools.lru_cache(maxsize=None)
def self_check():
    assert on_curve(G2) and compress(G2) == G2_COMPRESSED and decode(G2_COMPRESSED) == G2
    assert in_g2(G2) and in_g2_psi(G2) and psi(G2) == neg(mul(BLS_X, G2))
    assert on_curve(psi(mul(5, G2))) and psi_constants()[0][0] == 0
    a = point_with_x((1, 0), 0) or point_with_x((2, 0), 0)
    assert mul(H2 * R, a) is None and not in_g2(a) and not in_g2_psi(a)
    pts = golden_g2_bytes()
    assert len(pts) == 65
    for b in pts:
        a = decode(b)
        assert compress(a) == b and in_g2(a) and in_g2_psi(a)
    assert decode(pts[0]) == G2
    return True
