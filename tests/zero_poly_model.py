"""Test infrastructure: the reference's ZeroPoly (blst/src/zero_poly.rs) and PolyRecover (blst/src/recovery.rs) restated
on Python integers over fk20_model.fft / root_of_order.  A polynomial is a list of integers mod R, lowest coefficient
first; a missing sample is None.  Errors are ValueError with the reference's message.  Every output is a field element
with one value (a monic product of linear factors, its transform, a quotient by a value that is never zero), so the
route is free: do_zero_poly_mul_partial is the reference's long multiplication statement by statement, the larger
products take a divide-and-conquer product by transforms.  tests/test_zero_poly_model_cpu.py pins it on the reference's
known answers and test programs; the GPU tests hold the library to it.  Never imported by the product."""
import fk20_model as FM

R = FM.R
SCALE_FACTOR = 5


def next_pow_of_2(x):
    n = 1
    while n < x:
        n *= 2
    return n


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


_roots = {}


def roots_of_unity(max_width):
    """the settings' table: max_width + 1 powers of the primitive max_width-th root (the last equals the first)"""
    if max_width not in _roots:
        w = FM.root_of_order(max_width)
        out = [1]
        for _ in range(max_width):
            out.append(out[-1] * w % R)
        _roots[max_width] = out
    return _roots[max_width]


def do_zero_poly_mul_partial(max_width, idxs, stride):
    """zero_poly.rs:56-89"""
    if not idxs:
        raise ValueError("idx array must not be empty")
    roots = roots_of_unity(max_width)
    coeffs = [-roots[idxs[0] * stride] % R]
    for i in range(1, len(idxs)):
        neg_di = -roots[idxs[i] * stride] % R
        coeffs.append((neg_di + coeffs[i - 1]) % R)
        for j in range(i - 1, 0, -1):
            coeffs[j] = (coeffs[j] * neg_di + coeffs[j - 1]) % R
        coeffs[0] = coeffs[0] * neg_di % R
    coeffs.append(1)
    return coeffs


def reduce_partials(max_width, domain_size, partials):
    """zero_poly.rs:91-153"""
    if not is_pow2(domain_size):
        raise ValueError("Expected domain size to be a power of 2")
    if not partials:
        raise ValueError("partials must not be empty")
    if any(len(p) == 0 for p in partials):
        raise ValueError("attempt to subtract with overflow: empty partial")  # the reference underflows there
    out_degree = sum(len(p) - 1 for p in partials)
    if out_degree + 1 > domain_size:
        raise ValueError("Out degree is longer than possible polynomial size in domain")
    if domain_size > max_width:
        raise ValueError("Domain size greater than fft_settings.max_width")
    w = FM.root_of_order(domain_size) if domain_size > 1 else 1
    ev = [1] * domain_size
    for p in partials:
        pe = FM.fft(list(p) + [0] * (domain_size - len(p)), w)
        ev = [a * b % R for a, b in zip(ev, pe)]
    return FM.ifft(ev, w)[:out_degree + 1]


def _mul(a, b):
    n = len(a) + len(b) - 1
    if min(len(a), len(b)) <= 16:
        out = [0] * n
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % R
        return out
    N = next_pow_of_2(n)
    w = FM.root_of_order(N)
    fa, fb = FM.fft(list(a) + [0] * (N - len(a)), w), FM.fft(list(b) + [0] * (N - len(b)), w)
    return FM.ifft([x * y % R for x, y in zip(fa, fb)], w)[:n]


def product_of_roots(rs):
    """prod (X - r), len(rs) + 1 coefficients; the empty product is 1"""
    if not rs:
        return [1]
    if len(rs) == 1:
        return [-rs[0] % R, 1]
    h = len(rs) // 2
    return _mul(product_of_roots(rs[:h]), product_of_roots(rs[h:]))


def zero_poly_via_multiplication(max_width, domain_size, missing):
    """zero_poly.rs:177-313 -> (zero_eval, zero_poly), both of domain_size elements; two empty lists for no index"""
    if not missing:
        return [], []
    if len(missing) >= domain_size:
        raise ValueError("Missing idxs greater than domain size")
    if domain_size > max_width:
        raise ValueError("Domain size greater than fft_settings.max_width")
    if not is_pow2(domain_size):
        raise ValueError("Domain size must be a power of 2")
    if any(i >= domain_size for i in missing):
        raise ValueError("index out of bounds: missing idx exceeds domain size")  # the reference's later stages misbehave there
    roots = roots_of_unity(max_width)
    stride = max_width // domain_size
    zp = product_of_roots([roots[i * stride] for i in missing])
    zp = zp + [0] * (domain_size - len(zp))
    return FM.fft(zp, roots[stride]), zp


def empty_product(domain_size):
    """what the library returns for an empty list: (all ones, 1 0 0 ...)"""
    return [1] * domain_size, [1] + [0] * (domain_size - 1)


def shift_poly(p, k):
    """recovery.rs:20-59: coefficient i times k^i — exponent i, not the i + 1 of Poly::scale"""
    out, power = [], 1
    for c in p:
        out.append(c * power % R)
        power = power * k % R
    return out


def recover_poly_coeffs_from_samples(max_width, samples):
    """recovery.rs:62-172; defined for any sample values.  No missing sample: ifft(samples) (the reference fails there)."""
    n = len(samples)
    if not is_pow2(n):
        raise ValueError("Samples must have a length that is a power of two")
    missing = [i for i, s in enumerate(samples) if s is None]
    if len(missing) > n // 2:
        raise ValueError("Impossible to recover, too many shards are missing")
    if n > max_width:
        raise ValueError("Supplied list is longer than the available max width")
    w = roots_of_unity(max_width)[max_width // n]
    if missing:
        zero_eval, zero_poly = zero_poly_via_multiplication(max_width, n, missing)
    else:
        zero_eval, zero_poly = empty_product(n)
    ez = [0 if s is None else s * z % R for s, z in zip(samples, zero_eval)]
    inv5 = pow(SCALE_FACTOR, R - 2, R)
    q1 = FM.fft(shift_poly(FM.ifft(ez, w), inv5), w)
    q2 = FM.fft(shift_poly(zero_poly, inv5), w)
    q3 = [a * pow(b, R - 2, R) % R for a, b in zip(q1, q2)]
    return shift_poly(FM.ifft(q3, w), SCALE_FACTOR)


def recover_poly_from_samples(max_width, samples):
    """recovery.rs:174-194"""
    coeffs = recover_poly_coeffs_from_samples(max_width, samples)
    return FM.fft(coeffs, roots_of_unity(max_width)[max_width // len(samples)])
