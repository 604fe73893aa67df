"""Python-integer model of batched KZG proof checking (kzgamd_kzg_check_batch, rust-kzg_amd/csrc/kzg.hip).

Tuple t is (commitment C_t, proof pi_t, shift x_t, n values ys_t); I_t is the interpolation polynomial of the values on
the coset x_t <w>: ifft(ys_t), coefficient i times x_t^-i (the constant y_t for n = 1).  The reference's check
e(C_t - [I_t(s)]G, G2) == e(pi_t, [s^n]G2 - [x_t^n]G2) with x_t^n moved to the G1 side and the tuples weighted by
rho_t = r^t is one statement about two points,

    L = sum rho_t C_t + sum rho_t x_t^n pi_t - [A(s)]G,  A = sum rho_t I_t,    P = sum rho_t pi_t,    e(L, G2) == e(P, [s^n]G2).

With the setup's known secret every supplied point is [scalar]G, so L = [l]G and P = [p]G with

    l = sum rho_t (c_t - I_t(s) + x_t^n q_t),    p = sum rho_t q_t

and the batch passes exactly when l == s^n p.  c_t and q_t are whatever scalars the supplied points carry and I_t comes
from the supplied values, valid or not: the model says what the library must compute, not only what it must conclude.
"""
import hashlib

from kzg_model import R, SECRET, coset_values, proof_scalar  # noqa: F401  (re-exported for the tests)
from kzg_model import evaluate, root_of_order

DOMAIN = b"KZGAMD_CHKBATCH1"


def interpolation(ys, x, w):
    """the n coefficients of I: I(x w^j) = ys[j], by the definition of the inverse transform (n^2 steps)"""
    n = len(ys)
    if n == 1:
        return [ys[0] % R]
    n_inv, w_inv, x_inv = pow(n, R - 2, R), pow(w, R - 2, R), pow(x, R - 2, R)
    wp = [pow(w_inv, k, R) for k in range(n)]  # w has order n
    return [sum(ys[j] * wp[i * j % n] for j in range(n)) * n_inv * pow(x_inv, i, R) % R for i in range(n)]


def weights(r, count):
    out, cur = [], 1
    for _ in range(count):
        out.append(cur)
        cur = cur * r % R
    return out


def aggregated_polynomial(tuples, n, r, w):
    """A = sum rho_t I_t, n coefficients; tuples = [(c, q, x, ys)]"""
    A = [0] * n
    for rho, (_, _, x, ys) in zip(weights(r, len(tuples)), tuples):
        for i, v in enumerate(interpolation(ys, x, w)):
            A[i] = (A[i] + rho * v) % R
    return A


def tuple_terms(c, q, x, ys, n, w=None, s=SECRET):
    """what tuple t adds to (l, p) per unit of its weight: (c - I(s) + x^n q, q)"""
    w = root_of_order(n) if w is None else w
    return (c - evaluate(interpolation(ys, x, w), s) + pow(x, n, R) * q) % R, q % R


def combine(terms, r):
    """(l, p) from the tuples' terms and the weights r^t"""
    l = p = 0
    for rho, (a, q) in zip(weights(r, len(terms)), terms):
        l = (l + rho * a) % R
        p = (p + rho * q) % R
    return l, p


def batch_scalars(tuples, n, r, w=None, s=SECRET):
    """(l, p): the scalars of L and P over the generator"""
    return combine([tuple_terms(c, q, x, ys, n, w, s) for c, q, x, ys in tuples], r)


def batch_passes(tuples, n, r, w=None, s=SECRET):
    l, p = batch_scalars(tuples, n, r, w, s)
    return l == pow(s, n, R) * p % R


def tuple_passes(c, q, x, ys, n, w=None, s=SECRET):
    """the reference's per-tuple equation: c - I(s) == q (s^n - x^n)"""
    w = root_of_order(n) if w is None else w
    return (c - evaluate(interpolation(ys, x, w), s)) % R == q * (pow(s, n, R) - pow(x, n, R)) % R


def challenge_bytes(commitments, proofs, xs, ys, n, count):
    """D: the domain, n and count as big-endian 64-bit integers, then the four buffers as the caller holds them"""
    assert len(commitments) == len(proofs) == 144 * count and len(xs) == 32 * count and len(ys) == 32 * count * n
    return DOMAIN + n.to_bytes(8, "big") + count.to_bytes(8, "big") + commitments + proofs + xs + ys


def challenge(commitments, proofs, xs, ys, n, count):
    """hash_to_bls_field of SHA-256(D): the digest as a big-endian integer mod R"""
    return int.from_bytes(hashlib.sha256(challenge_bytes(commitments, proofs, xs, ys, n, count)).digest(), "big") % R
