"""Python-integer model of kzgamd_verify_cell_kzg_proof_batch_many (rust-kzg_amd/csrc/ckzg_vcells.hip).

The EIP-7594 structure with free sizes: a cell has n field elements, an extended blob K cells (the product: n = 64,
K = 128), the domain is the n K-th roots of unity with generator w, a polynomial has n K / 2 coefficients.  Cell k holds
the values of p on the coset h_k <w^K>, h_k = w^brev(k), element j at h_k (w^K)^brev(j) (bit-reversed inside the cell,
kzg/src/das.rs:267-275); its proof commits to (p - I_k) / (X^n - h_k^n), I_k the interpolation polynomial of the cell.

With the setup's known secret s every supplied point is [scalar]G.  One batch of (commitment c_i, column k_i, cell values,
proof q_i), i < m, with the challenge r, is accepted by the reference (das.rs:294-389) when l == s^n p for

    p = sum r^i q_i,        l = sum r^i c_i - sum r^i I_i(s) + sum r^i h_{k_i}^n q_i

(`batch_pair`; I_i from the SUPPLIED values, valid or not).  The call over B batches with outer weights rho^b computes,
from the cell weights w_i = rho^b r_b^i alone (`call_pair`):

    one weight per distinct commitment of the whole call (the sum of the w_i that name it),
    one aggregated vector per column, agg[k][j] = sum over the cells i of column k of w_i cell_i[j],
    ONE interpolation polynomial A of n coefficients, A_t = sum_k ifft(agg[k])_t h_k^-t,
    p = sum w_i q_i,        l = sum_g W_g c_g - A(s) + sum_i w_i h_{k_i}^n q_i

and must equal sum_b rho^b (p_b, l_b).
"""
import hashlib

from fk20_model import R, SECRET, brev, ifft, root_of_order  # noqa: F401  (re-exported for the tests)
from kzg_model import evaluate, long_division

DOMAIN = b"KZGAMD_VCELLSET1"


class Shape:
    def __init__(self, n, K):
        self.n, self.K = n, K
        self.w = root_of_order(n * K)
        self.wn = pow(self.w, K, R)  # generator of the cells' subgroup of order n
        self.nbits, self.kbits = n.bit_length() - 1, K.bit_length() - 1

    def h(self, k):
        return pow(self.w, brev(k, self.kbits), R)

    def cell(self, p, k):
        """the n values of cell k of polynomial p, in the cell's own (bit-reversed) order"""
        hk = self.h(k)
        return [evaluate(p, hk * pow(self.wn, brev(j, self.nbits), R) % R) for j in range(self.n)]

    def proof_scalar(self, p, k, s=SECRET):
        c = pow(self.h(k), self.n, R)
        _, rem = long_division(p, self.n, c)
        return (evaluate(p, s) - evaluate(rem, s)) * pow((pow(s, self.n, R) - c) % R, R - 2, R) % R

    def interpolation(self, values, k):
        """the n coefficients of the polynomial with `values` (cell order) on the coset of column k"""
        nat = [0] * self.n
        for j, v in enumerate(values):
            nat[brev(j, self.nbits)] = v % R
        co = ifft(nat, self.wn)
        hinv = pow(self.h(k), R - 2, R)
        return [c * pow(hinv, t, R) % R for t, c in enumerate(co)]


def batch_pair(sh, cells, r, s=SECRET):
    """(p, l) of one batch, the reference's formulas; cells = [(c, k, values, q)]"""
    p = l = 0
    w = 1
    for c, k, values, q in cells:
        p = (p + w * q) % R
        l = (l + w * (c - evaluate(sh.interpolation(values, k), s) + pow(sh.h(k), sh.n, R) * q)) % R
        w = w * r % R
    return p, l


def batch_passes(sh, cells, r, s=SECRET):
    p, l = batch_pair(sh, cells, r, s)
    return l == pow(s, sh.n, R) * p % R


def call_pair(sh, batches, rs, rho, s=SECRET):
    """(p, l) of the whole call as the library computes it; batches = [cells], rs = [r_b]; a commitment is identified
    by its scalar (the library: by its 48 bytes)"""
    weight = {}                      # global commitment weights, first occurrences in order
    agg = {}                         # column -> n sums
    p = lp = 0
    rho_b = 1
    for cells, r in zip(batches, rs):
        w = rho_b
        for c, k, values, q in cells:
            weight[c] = (weight.get(c, 0) + w) % R
            row = agg.setdefault(k, [0] * sh.n)
            for j, v in enumerate(values):
                row[j] = (row[j] + w * v) % R
            p = (p + w * q) % R
            lp = (lp + w * pow(sh.h(k), sh.n, R) * q) % R
            w = w * r % R
        rho_b = rho_b * rho % R
    A = [0] * sh.n
    for k, row in agg.items():
        for t, v in enumerate(sh.interpolation(row, k)):
            A[t] = (A[t] + v) % R
    l = (sum(wt * c for c, wt in weight.items()) - evaluate(A, s) + lp) % R
    return p, l


def call_passes(sh, batches, rs, rho, s=SECRET):
    p, l = call_pair(sh, batches, rs, rho, s)
    return l == pow(s, sh.n, R) * p % R


def outer_challenge_bytes(rs):
    """the domain, the number of batches as a big-endian 64-bit integer, then every r_b as 32 big-endian bytes"""
    return DOMAIN + len(rs).to_bytes(8, "big") + b"".join((r % R).to_bytes(32, "big") for r in rs)


def outer_challenge(rs):
    """hash_to_bls_field of SHA-256 of those bytes: the digest as a big-endian integer mod R"""
    return int.from_bytes(hashlib.sha256(outer_challenge_bytes(rs)).digest(), "big") % R
