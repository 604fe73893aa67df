"""Python-integer model of what kzgamd_g1_mul_batch / kzgamd_g2_mul_batch / kzgamd_generate_trusted_setup compute: the
scalar cases the GPU tests run, hash_to_bls_field, and the closed forms of a generated setup.

  g1_monomial[i] = [s^i]G1, g2_monomial[j] = [s^j]G2, g1_lagrange[i] = [L_i(s)]G1 with
  L_i(s) = (1/n) sum_j s^j w^(-ij)   (the inverse transform of the powers, natural order; w the n-th root of the handle)

tests/test_setup_model_cpu.py pins the model against itself; the GPU tests hold the library to it ([scalar]G by the CPU
oracle, [scalar]G2 by the host's kzgamd_p2_mult).  Never imported by the product."""
import random

import fk20_model as M

R = M.R


def scalar_cases():
    """Scalars below r that reach every digit and carry edge of a windowed walk of ANY width, signed or unsigned: the
    list does not know the library's window.  Order is fixed; duplicates are removed."""
    out = [0, 1, 2, R - 1, R - 2, (1 << 254) - 1]
    for k in range(255):
        for v in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            if v < R:
                out.append(v)
    for w in range(2, 17):
        for digit in ((1 << w) - 1, 1 << (w - 1), (1 << (w - 1)) - 1, (1 << (w - 1)) + 1):
            v = 0
            for pos in range(0, 254 + w, w):
                v |= digit << pos
            v &= (1 << 254) - 1  # truncated to 254 bits: below r
            out.append(v)
    rnd = random.Random(0x5E7)
    out += [rnd.randrange(R) for _ in range(64)]
    seen, uniq = set(), []
    for v in out:
        assert 0 <= v < R
        if v not in seen:
            seen.add(v)
            uniq.append(v)
    return uniq


def family_2k():
    """{value: k} for the 2^k - 1, 2^k, 2^k + 1 family of scalar_cases (the part a slow reference may thin out)"""
    out = {}
    for k in range(255):
        for v in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            if v < R:
                out.setdefault(v, k)
    return out


def hash_to_bls_field(secret: bytes) -> int:
    """kzg/src/eip_4844.rs hash_to_bls_field: the 32 bytes as a big-endian integer, reduced mod r"""
    assert len(secret) == 32
    return int.from_bytes(secret, "big") % R


SECRETS = {
    "ff": b"\xff" * 32,  # at least r: pins the reduction
    "zero": bytes(32),
    "one": (1).to_bytes(32, "big"),
    "fk20": M.SECRET.to_bytes(32, "big"),
}


def powers(s, n):
    out, v = [], 1
    for _ in range(n):
        out.append(v)
        v = v * s % R
    return out


def lagrange_closed_form(s, n, w):
    """L_i(s) = (1/n) sum_j s^j w^(-ij), i < n"""
    n_inv, w_inv, p = pow(n, R - 2, R), pow(w, R - 2, R), powers(s, n)
    return [n_inv * sum(p[j] * pow(w_inv, i * j, R) for j in range(n)) % R for i in range(n)]


def lagrange_by_ifft(s, n, w):
    return M.ifft(powers(s, n), w) if n > 1 else [1]
