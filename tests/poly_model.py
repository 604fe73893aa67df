"""Test infrastructure: the reference's Poly<Fr> (blst/src/types/poly.rs) restated on Python integers, statement by
statement where the statement matters (the exponent of scale, the precision sequence of inverse, the thresholds of mul
and div).  A polynomial is a list of integers mod R, lowest coefficient first.  Errors are ValueError with the
reference's message.  tests/test_poly_model_cpu.py pins it on the reference's own test programs; the GPU tests hold the
library to it.  Never imported by the product."""
import fk20_model as FM

R = FM.R
SCALE_FACTOR = 5


def next_pow_of_2(x):
    n = 1
    while n < x:
        n *= 2
    return n


def evaluate(p, x):
    """Poly::eval, poly.rs:42-62"""
    if not p:
        return 0
    if x == 0:
        return p[0]
    ret = p[-1]
    for c in reversed(p[:-1]):
        ret = (ret * x + c) % R
    return ret


def scale(p):
    """poly.rs:64-73: the power is multiplied BEFORE it is used, so coefficient i gets 5^-(i+1)"""
    inv = pow(SCALE_FACTOR, R - 2, R)
    out, power = [], 1
    for c in p:
        power = power * inv % R
        out.append(c * power % R)
    return out


def unscale(p):
    """poly.rs:75-83"""
    out, power = [], 1
    for c in p:
        power = power * SCALE_FACTOR % R
        out.append(c * power % R)
    return out


def mul_direct(a, b, output_len):
    """poly.rs:252-277"""
    if not a or not b:
        return []
    ret = [0] * output_len
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            if i + j >= output_len:
                break
            ret[i + j] = (ret[i + j] + ai * bj) % R
    return ret


def mul_fft(a, b, output_len):
    """poly.rs:340-396, over fk20_model.fft"""
    length = next_pow_of_2(len(a) + len(b) - 1)
    w = FM.root_of_order(length)
    fa = FM.fft(list(a) + [0] * (length - len(a)), w)
    fb = FM.fft(list(b) + [0] * (length - len(b)), w)
    ab = FM.ifft([x * y % R for x, y in zip(fa, fb)], w)
    ret = [0] * output_len
    n = min(output_len, length)
    ret[:n] = ab[:n]
    return ret


def mul(a, b, output_len):
    """poly.rs:398-405"""
    if len(a) < 64 or len(b) < 64 or output_len < 128:
        return mul_direct(a, b, output_len)
    return mul_fft(a, b, output_len)


def precision_sequence(output_len):
    """the values d takes in Poly::inverse (poly.rs:118-122); the last is output_len - 1"""
    maxd = output_len - 1
    out, d = [], 0
    mask = 1 << (maxd.bit_length() - 1) if maxd else 0
    while mask:
        d = 2 * d + (1 if maxd & mask else 0)
        mask >>= 1
        out.append(d)
    return out


def inverse(b, output_len):
    """poly.rs:86-149"""
    if output_len == 0:
        raise ValueError("Can't produce a zero-length result")
    if not b:
        raise ValueError("Can't inverse a zero-length poly")
    if b[0] == 0:
        raise ValueError("First coefficient of polynomial mustn't be zero")
    ret = [0] * output_len
    ret[0] = pow(b[0], R - 2, R)
    if len(b) == 1:
        return ret
    d = 0
    for d in precision_sequence(output_len):
        len_temp = min(d + 1, len(b) + output_len - 1)
        tmp0 = mul(b, ret, len_temp)
        tmp0 = [(-v) % R for v in tmp0]
        tmp0[0] = (tmp0[0] + 2) % R
        tmp1 = mul(ret, tmp0, d + 1)
        ret[:len(tmp1)] = tmp1
    if d + 1 != output_len:
        raise ValueError("D + 1 must be equal to output_len")
    return ret


def inverse_recurrence(b, output_len):
    """the same series by c_j = -c_0 sum_{i >= 1} b_i c_{j-i}: an independent anchor for short outputs"""
    c0 = pow(b[0], R - 2, R)
    c = [c0]
    for j in range(1, output_len):
        acc = sum(b[i] * c[j - i] for i in range(1, min(j, len(b) - 1) + 1)) % R
        c.append((-c0 * acc) % R)
    return c


def _check_divisor(b):
    if not b:
        raise ValueError("Can't divide by zero")
    if b[-1] == 0:
        raise ValueError("Highest coefficient must be non-zero")


def long_div(a, b):
    """poly.rs:160-214"""
    _check_divisor(b)
    out_length = len(a) - len(b) + 1 if len(a) >= len(b) else 0
    if out_length == 0:
        return []
    if len(b) == 2:
        inv1 = pow(b[1], R - 2, R)
        out = list(a[1:])
        for i in range(out_length - 1, 0, -1):
            out[i] = out[i] * inv1 % R
            out[i - 1] = (out[i - 1] - out[i] * b[0]) % R
        out[0] = out[0] * inv1 % R
        return out
    out = [0] * out_length
    a = list(a)
    a_pos, b_pos = len(a) - 1, len(b) - 1
    diff = a_pos - b_pos
    inv = pow(b[b_pos], R - 2, R)
    while diff > 0:
        out[diff] = a[a_pos] * inv % R
        for i in range(b_pos + 1):
            a[diff + i] = (a[diff + i] - out[diff] * b[i]) % R
        diff -= 1
        a_pos -= 1
    out[0] = a[a_pos] * inv % R
    return out


def fast_div(a, b):
    """poly.rs:216-250"""
    _check_divisor(b)
    m, n = len(a) - 1, len(b) - 1
    if n > m:
        return []
    if len(b) == 1:
        inv = pow(b[0], R - 2, R)
        return [v * inv % R for v in a]
    a_flip, b_flip = a[::-1], b[::-1]
    inv_b_flip = inverse(b_flip, m - n + 1)
    q_flip = mul(a_flip, inv_b_flip, m - n + 1)
    return q_flip[::-1]


def div(a, b):
    """poly.rs:151-158"""
    if len(b) >= len(a) or len(b) < 128:
        return long_div(a, b)
    return fast_div(a, b)
