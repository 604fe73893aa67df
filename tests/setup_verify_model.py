"""Python-integer model of kzgamd_verify_trusted_setup: the four checks over discrete logarithms.

A point of G1 or G2 is the integer k of [k]G1 / [k]G2 (mod r; 0 is the identity), a pairing e([a]G1, [b]G2) is a * b in
the exponent, so e(X, Y) == e(Z, W) is x y == z w (mod r) — which is also what the library's pairing check gives when a
side holds an identity (that side is skipped: exponent 0).  A setup is (m, l, q): the logarithms of g1_monomial,
g1_lagrange (natural order; None: not given) and g2_monomial.

  challenge(seed)        hash_to_bls_field of the 32 bytes, 0 replaced by 1
  derive_seed(...)       the 32 bytes the library takes for seed == NULL, from the compressed points
  failed_bits(...)       the bits of the checks that fail:
      1  m[0] == 1 and q[0] == 1
      2  B q[0] == A q[1]   with A = sum_{i < n1 - 1} r^i m[i],  B = sum_{i < n1 - 1} r^i m[i + 1]
      4  m[1] C == m[0] D   with C = sum_{j < n2 - 1} r^j q[j],  D = sum_{j < n2 - 1} r^j q[j + 1]
      8  sum_i f[i] l[i] == sum_k r^k m[k]   with f the forward transform of (r^0 ... r^(n1 - 1)) by the root w
  make_setup / the tampers of the GPU test, each on logarithms

Never imported by the product."""
import hashlib

import fk20_model as M
import setup_model as S

R = M.R
DOMAIN = b"KZGAMD_VERIFY_SETUP_V1"


def challenge(seed: bytes) -> int:
    return S.hash_to_bls_field(seed) or 1


def derive_seed(num_g1, num_g2, m_bytes, l_bytes, q_bytes) -> bytes:
    """m_bytes / l_bytes: 48 * num_g1 bytes of compressed G1 points (l_bytes None without L), q_bytes: 96 * num_g2"""
    assert len(m_bytes) == 48 * num_g1 and len(q_bytes) == 96 * num_g2 and (l_bytes is None or len(l_bytes) == 48 * num_g1)
    h = hashlib.sha256()
    h.update(DOMAIN + num_g1.to_bytes(8, "big") + num_g2.to_bytes(8, "big") + (b"\x00" if l_bytes is None else b"\x01"))
    h.update(m_bytes)
    if l_bytes is not None:
        h.update(l_bytes)
    h.update(q_bytes)
    return h.digest()


def make_setup(s, n1, n2, w=None):
    """(m, l, q) of the secret s; l None when no root w is given"""
    m, q = S.powers(s, n1), S.powers(s, n2)
    return m, (S.lagrange_by_ifft(s, n1, w) if w is not None else None), q


def failed_bits(m, l, q, r, w=None):
    n1, n2 = len(m), len(q)
    assert n1 >= 2 and n2 >= 2
    pw = S.powers(r, max(n1, n2))
    bad = 0
    if m[0] % R != 1 or q[0] % R != 1:
        bad |= 1
    A = sum(pw[i] * m[i] for i in range(n1 - 1)) % R
    B = sum(pw[i] * m[i + 1] for i in range(n1 - 1)) % R
    if (B * q[0] - A * q[1]) % R:
        bad |= 2
    Cc = sum(pw[j] * q[j] for j in range(n2 - 1)) % R
    D = sum(pw[j] * q[j + 1] for j in range(n2 - 1)) % R
    if (m[1] * Cc - m[0] * D) % R:
        bad |= 4
    if l is not None:
        assert len(l) == n1 and n1 & (n1 - 1) == 0 and w is not None
        f = M.fft(pw[:n1], w) if n1 > 1 else pw[:1]
        if (sum(a * b for a, b in zip(f, l)) - sum(pw[k] * m[k] for k in range(n1))) % R:
            bad |= 8
    return bad


def bit_reverse(v):
    bits = len(v).bit_length() - 1
    return [v[M.brev(i, bits)] for i in range(len(v))]


OTHER = 0x1234567890ABCDEF  # the logarithm of "another point of G1 / G2"


def tampers(n1, n2):
    """{name: function (m, l, q, s2) -> (m, l, q)} on copies; s2: a setup (m, l, q) of another secret, the same sizes"""
    def replace_m(k):
        def f(m, l, q, s2):
            m = list(m)
            m[k] = OTHER
            return m, l, q
        return f

    def replace_q(j):
        def f(m, l, q, s2):
            q = list(q)
            q[j] = OTHER
            return m, l, q
        return f

    def swap_m(m, l, q, s2):
        m = list(m)
        m[3], m[n1 - 2] = m[n1 - 2], m[3]
        return m, l, q

    def replace_l(m, l, q, s2):
        l = list(l)
        l[n1 // 2 + 1] = OTHER
        return m, l, q

    out = {"M[%d] replaced" % k: replace_m(k) for k in (0, 1, n1 // 2, n1 - 1)}
    out["two M entries swapped"] = swap_m
    out.update({"Q[%d] replaced" % j: replace_q(j) for j in (1, n2 - 1)})
    out["one L entry replaced"] = replace_l
    out["L in bit-reversed order"] = lambda m, l, q, s2: (m, bit_reverse(l), q)
    out["G1 and G2 sides of different secrets"] = lambda m, l, q, s2: (m, l, s2[2])
    out["every M scaled by one constant"] = lambda m, l, q, s2: ([7 * v % R for v in m], l, q)
    return out


# what each tamper must report with L given (without L: the same less bit 8), for ANY challenge outside a set of
# probability <= (2 n1 + n2) / r; tests/test_setup_verify_model_cpu.py derives the same bits from failed_bits
def expected_bits(name, n1):
    if name == "M[0] replaced":
        return 1 | 2 | 4 | 8
    if name == "M[1] replaced":
        return 2 | 4 | 8
    if name.startswith("M[") or name == "two M entries swapped":
        return 2 | 8
    if name.startswith("Q[") and name != "Q[1] replaced":
        return 4
    if name == "Q[1] replaced":
        return 2 | 4
    if name in ("one L entry replaced", "L in bit-reversed order"):
        return 8
    if name == "G1 and G2 sides of different secrets":
        return 2 | 4
    if name == "every M scaled by one constant":
        return 1 | 8  # both pairing checks are homogeneous in M: only the generator and the Lagrange form notice
    raise KeyError(name)
