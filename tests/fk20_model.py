"""Test infrastructure: FK20 data-availability proofs on Python integers, two ways.

* `fk20_restated`: the reference's algorithm (FK20SingleSettings / FK20MultiSettings::data_availability_optimized,
  blst/src/types/fk20_multi_settings.rs:60-175, toeplitz_part_1/2/3 and toeplitz_coeffs_stride,
  blst/src/fk20_proofs.rs:16-93) with G1 replaced by Fr: the generator is 1, the setup point [s^i]G is s^i, so every
  "proof" is the discrete logarithm of the reference's proof.
* `fk20_closed_form`: what those proofs are, with the secret s known.  With l = chunk_len, k2 = 2n / l and
  c_j = w^j (w of order k2), entry j of the optimized output is
      (p(s) - I_j(s)) / (s^l - c_j),   I_j = p mod (X^l - c_j),   coefficient t of I_j = sum_b p[b l + t] c_j^b,
  the KZG multi-proof of the coset { x : x^l = c_j }.  All I_j(s) come from l transforms of size k2.

tests/test_fk20_model_cpu.py holds the two equal; the GPU tests hold the library to the closed form ([scalar]G from the
CPU oracle).  Never imported by the product."""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
# the secret of the reference's FK20 tests and bench (kzg-bench/src/tests/fk20_proofs.rs:6-9), little-endian
SECRET = int.from_bytes(bytes([0xA4, 0x73, 0x31, 0x95, 0x28, 0xC8, 0xB6, 0xEA, 0x4D, 0x08, 0xCC, 0x53, 0x18] + [0] * 19), "little")


def brev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def root_of_order(n):
    """a primitive n-th root of unity (n a power of two up to 2^32); 7 generates the multiplicative group"""
    return pow(7, (R - 1) // n, R)


def fft(vals, w):
    """iterative radix-2, natural order in and out: out[k] = sum_j vals[j] w^(jk), w of order len(vals)"""
    n = len(vals)
    bits = n.bit_length() - 1
    a = [vals[brev(i, bits)] for i in range(n)]
    m = 2
    while m <= n:
        wm = pow(w, n // m, R)
        tw = [1] * (m // 2)
        for j in range(1, m // 2):
            tw[j] = tw[j - 1] * wm % R
        for k in range(0, n, m):
            for j in range(m // 2):
                t = tw[j] * a[k + j + m // 2] % R
                u = a[k + j]
                a[k + j] = (u + t) % R
                a[k + j + m // 2] = (u - t) % R
        m *= 2
    return a


def ifft(vals, w):
    n_inv = pow(len(vals), R - 2, R)
    return [v * n_inv % R for v in fft(vals, pow(w, R - 2, R))]


def toeplitz_coeffs_stride(p, offset, stride):
    """fk20_proofs.rs:65-88, statement by statement"""
    n = len(p)
    k = n // stride
    k2 = 2 * k
    ret = [p[n - 1 - offset]]
    num_of_zeroes = k + 2 - 1 if k + 2 < k2 else k2 - 1
    ret += [0] * num_of_zeroes
    i, j = k + 2, 2 * stride - offset - 1
    while i < k2:
        ret.append(p[j])
        i += 1
        j += stride
    return ret


def fk20_restated(p, chunk_len, s, w):
    """data_availability_optimized with scalars for points; w: the root of order k2 = 2 len(p) / chunk_len"""
    n, l = len(p), chunk_len
    k = n // l
    k2 = 2 * k
    files = []
    for offset in range(l):  # FK20MultiSettings::new (the single form is l = 1: x[i] = s^(n - 2 - i))
        start = n - l - 1 - offset if n >= l + 1 + offset else 0
        x, j = [], start
        for _ in range(k - 1):
            x.append(pow(s, j, R))
            j = j - l if j >= l else 0
        x.append(0)
        files.append(fft(x + [0] * (k2 - k), w))  # toeplitz_part_1
    h_ext = [0] * k2
    for i in range(l):
        c = fft(toeplitz_coeffs_stride(p, i, l), w)  # toeplitz_part_2
        for j in range(k2):
            h_ext[j] = (h_ext[j] + c[j] * files[i][j]) % R
    h = ifft(h_ext, w)  # toeplitz_part_3
    h[k:] = [0] * (k2 - k)
    return fft(h, w)


def fk20_closed_form(p, chunk_len, s, w):
    n, l = len(p), chunk_len
    k = n // l
    k2 = 2 * k
    ps = 0
    for c in reversed(p):
        ps = (ps * s + c) % R
    interp = [0] * k2  # I_j(s)
    st = 1
    for t in range(l):
        col = fft([p[b * l + t] for b in range(k)] + [0] * k, w)
        for j in range(k2):
            interp[j] = (interp[j] + st * col[j]) % R
        st = st * s % R
    sl = pow(s, l, R)
    out, c = [], 1
    for j in range(k2):
        out.append((ps - interp[j]) * pow((sl - c) % R, R - 2, R) % R)
        c = c * w % R
    return out


def fk_single_poly():
    """fk_single / fk_single_strided of the reference (kzg-bench/src/tests/fk20_proofs.rs:28, 92)"""
    return [1, 2, 3, 4, 7, 7, 7, 7, 13, 13, 13, 13, 13, 13, 13, 13]


def fk_multi_poly(n, chunk_len):
    """the polynomial of fk_multi_case (kzg-bench/src/tests/fk20_proofs.rs:174-213)"""
    vv = [1, 2, 3, 4, 7, 8, 9, 10, 13, 14, 1, 15, 1, 1000, 134, 33]
    p = [0] * n
    for i in range(n // chunk_len):
        for j in range(chunk_len):
            pi = i * chunk_len + j
            vi = pi % 16
            v = vv[vi]
            tmp = i * chunk_len // 16
            if vi == 3:
                v += tmp
            if vi == 5:
                v += tmp * tmp
            p[pi] = v % R
            if vi in (12, 14):
                p[pi] = (-p[pi]) % R
    return p
