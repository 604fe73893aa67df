"""Python-integer models of the quotient of generic polynomial KZG (rust-kzg_amd/csrc/kzg.hip).

p = q (X^n - c) + r with c = x^n, deg r < n.  With h_j = p_j + c h_{j+n} (h_j = 0 beyond the polynomial) the quotient is
q_j = h_{j+n} and the remainder r_j = h_j for j < n: one first-order recurrence per residue rho = j mod n, over the
sequence a_t = p_{rho + t n}, run from the top.

  chunked_quotient   the algorithm exactly as the kernels run it: every lane takes `chunk` consecutive steps of a sequence
                     from a zero carry (S_m), a log-step suffix scan with the powers (c^chunk)^(2^k) over the lanes of a
                     wave of `wave` lanes gives the values at the chunk bases, the waves of a sequence are chained through
                     one summary each — the same scan, a lane per wave, with the powers of (c^chunk)^wave, in blocks of
                     `wave` summaries from the top — and every chunk is replayed from its true incoming carry
  long_division      schoolbook division by X^n - c
  closed forms       with the setup's secret s: commitment scalar p(s), proof scalar (p(s) - r(s)) / (s^n - x^n), and the
                     values p(x w^i) by direct evaluation
"""
from fk20_model import R, SECRET, root_of_order  # noqa: F401  (re-exported for the tests)


def evaluate(p, x):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % R
    return acc


def long_division(p, n, c):
    """(q, r) with p = q (X^n - c) + r, len(q) = max(len(p) - n, 0), len(r) = n (zero-extended)"""
    rem = list(p)
    L = max(len(p) - n, 0)
    q = [0] * L
    for j in range(L - 1, -1, -1):
        q[j] = rem[j + n] % R
        rem[j + n] = 0
        rem[j] = (rem[j] + c * q[j]) % R
    r = [v % R for v in rem[:n]] + [0] * max(0, n - len(rem))
    return q, r[:n]


def chunked_quotient(p, n, c, chunk, wave=64):
    """(q, r) as long_division, by the kernels' three steps: local pass, scan with the power table, replay"""
    ln = len(p)
    L = max(ln - n, 0)
    q, r = [0] * L, [0] * n
    T = -(-ln // n)
    M = -(-T // chunk)
    gw = 1
    while gw < wave and gw < M:
        gw *= 2
    wv = -(-M // wave) if M > wave else 1
    slots = gw * wv
    C = pow(c, chunk, R)
    lw = wave.bit_length() - 1
    powers = [pow(C, 1 << k, R) for k in range(2 * lw)]  # C^(2^k); powers[lw + k] = (C^wave)^(2^k)
    for rho in range(n):

        def a(t):
            j = rho + t * n
            return p[j] if j < ln else None

        # local pass: every chunk from a zero carry
        S = [0] * slots
        for m in range(M):
            acc = 0
            for i in range(chunk - 1, -1, -1):
                v = a(m * chunk + i)
                if v is not None:
                    acc = (v + c * acc) % R
            S[m] = acc

        def scan(vals, width=gw, first=0):
            H = list(vals)
            k = 0
            while (1 << k) < width:
                H = [(H[i] + powers[first + k] * H[i + (1 << k)]) % R if i + (1 << k) < width else H[i] for i in range(width)]
                k += 1
            return H

        # the waves' summaries, then the true values at the wave bases (the second launch: blocks of `wave` summaries)
        G = [scan(S[w * gw:(w + 1) * gw])[0] for w in range(wv)]
        if wv > 1:
            carry = 0
            for blk in range(-(-wv // wave) - 1, -1, -1):
                vals = [G[blk * wave + i] if blk * wave + i < wv else 0 for i in range(wave)]
                vals[wave - 1] = (vals[wave - 1] + powers[lw] * carry) % R
                H = scan(vals, wave, lw)
                for i in range(wave):
                    if blk * wave + i < wv:
                        G[blk * wave + i] = H[i]
                carry = H[0]
        # the last launch: scan again from the value above the wave, replay
        for w in range(wv):
            above = G[w + 1] if w + 1 < wv else 0
            vals = S[w * gw:(w + 1) * gw]
            if w + 1 < wv:
                vals[gw - 1] = (vals[gw - 1] + C * above) % R
            H = scan(vals)
            for lane in range(gw):
                m = w * gw + lane
                if m >= M:
                    continue
                acc = H[lane + 1] if lane + 1 < gw else above
                for i in range(chunk - 1, -1, -1):
                    t = m * chunk + i
                    v = a(t)
                    if v is None:
                        continue
                    acc = (v + c * acc) % R
                    j = rho + t * n
                    if j >= n:
                        q[j - n] = acc
                    else:
                        r[rho] = acc
    return q, r


def commitment_scalar(p, s=SECRET):
    return evaluate(p, s)


def proof_scalar(p, x, n, s=SECRET):
    """(p(s) - r(s)) / (s^n - x^n) with r the remainder of p by X^n - x^n"""
    c = pow(x, n, R)
    _, r = long_division(p, n, c)
    den = (pow(s, n, R) - c) % R
    return (evaluate(p, s) - evaluate(r, s)) * pow(den, R - 2, R) % R


def coset_values(p, x, n, w):
    """p(x w^i), i < n, by direct evaluation"""
    return [evaluate(p, x * pow(w, i, R) % R) for i in range(n)]
