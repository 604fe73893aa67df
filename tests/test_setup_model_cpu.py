"""tests/setup_model.py pinned against itself on the CPU, and the entry points of the batched group multiplication named by
the header, the library, the Python module and the Rust sys crate.  No GPU: the answers asked of the library here are the
ones it gives before it touches a device (counts of zero, NULL arguments, the tuning string, a base at infinity, a base
outside the subgroup)."""
import ctypes as C
import os

import fk20_model as M
import g1_encodings as E
import setup_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = S.R
NAMES = ("kzgamd_g1_mul_batch", "kzgamd_g2_mul_batch", "kzgamd_generate_trusted_setup", "kzgamd_group_mul_info")


def test_scalar_cases_cover_the_digit_and_carry_edges_of_any_window():
    cases = S.scalar_cases()
    assert len(cases) == len(set(cases)) and all(0 <= v < R for v in cases)
    assert cases[:6] == [0, 1, 2, R - 1, R - 2, (1 << 254) - 1]
    assert 800 <= len(cases) <= 1000
    for k in range(254):
        assert {(1 << k) - 1, 1 << k, (1 << k) + 1} <= set(cases), k
    assert (1 << 254) + 1 in cases and (1 << 254) in cases
    for w in range(2, 17):
        nd = 254 // w  # whole digits below the truncation
        for digit in ((1 << w) - 1, 1 << (w - 1), (1 << (w - 1)) - 1, (1 << (w - 1)) + 1):
            hit = [v for v in cases if all((v >> (w * i)) & ((1 << w) - 1) == digit for i in range(nd))]
            assert hit, (w, digit)
    # every signed base-256 digit value from -128 to 128 occurs somewhere, and so does a carry into the top window
    digits = set()
    for v in cases:
        carry = 0
        for i in range(32):
            d = ((v >> (8 * i)) & 0xff) + carry
            carry = 1 if d > 128 else 0
            digits.add(d - 256 if carry else d)
        assert carry == 0, hex(v)
    assert {-128 + 1, -1, 0, 1, 127, 128} <= digits
    assert len(S.family_2k()) >= 750 and all(v in set(cases) for v in S.family_2k())


def test_hash_to_bls_field_reduces_mod_r():
    assert S.hash_to_bls_field(S.SECRETS["ff"]) == ((1 << 256) - 1) % R != (1 << 256) - 1
    assert S.hash_to_bls_field(S.SECRETS["zero"]) == 0 and S.hash_to_bls_field(S.SECRETS["one"]) == 1
    assert S.hash_to_bls_field(S.SECRETS["fk20"]) == M.SECRET % R == M.SECRET
    assert S.hash_to_bls_field(R.to_bytes(32, "big")) == 0 and S.hash_to_bls_field((R + 5).to_bytes(32, "big")) == 5


def test_inverse_fft_of_the_powers_is_the_closed_form():
    for name, secret in S.SECRETS.items():
        s = S.hash_to_bls_field(secret)
        for n in (1, 2, 4, 16, 64):
            w = M.root_of_order(n)
            assert pow(w, n, R) == 1 and (n == 1 or pow(w, n // 2, R) == R - 1)
            got, want = S.lagrange_by_ifft(s, n, w), S.lagrange_closed_form(s, n, w)
            assert got == want, (name, n)
            assert sum(got) % R == 1  # the Lagrange basis sums to one: the coefficient of s^0 after the forward transform
            assert M.fft(got, w) == S.powers(s, n) if n > 1 else got == [1]
    # secret zero: L_i = 1/n for every i; secret one: L_0 = 1, the rest 0
    assert S.lagrange_closed_form(0, 8, M.root_of_order(8)) == [pow(8, R - 2, R)] * 8
    assert S.lagrange_closed_form(1, 8, M.root_of_order(8)) == [1] + [0] * 7


def test_header_library_python_module_and_rust_sys_crate_name_the_entry_points():
    from conftest import load_package
    from test_host_cpu import _c_prototypes, _rust_externs

    protos = _c_prototypes()
    ext = _rust_externs(os.path.join(ROOT, "rust-kzg_amd", "rust", "src", "lib.rs"))
    pkg = load_package("product")
    L = pkg.lib()
    for name, nargs in zip(NAMES, (5, 5, 8, 3)):
        assert len(protos[name]) == nargs, (name, protos[name])
        assert len(ext[name]) == nargs, (name, ext[name])
        assert name in pkg.EXPORTS and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    for fn in ("g1_mul_batch", "g2_mul_batch", "generate_trusted_setup", "group_mul_info"):
        assert callable(getattr(pkg, fn)), fn
    info = pkg.group_mul_info()
    assert info["slice_points"] >= 64 and info["slice_points"] & (info["slice_points"] - 1) == 0
    assert 2 <= info["g1_window_bits"] <= 16 and 2 <= info["g2_window_bits"] <= 16
    assert "mul_slice" not in pkg.tuning_keys()


def test_answers_given_before_a_device_is_touched():
    from conftest import load_package

    pkg = load_package("product")
    L = pkg.lib()
    one = (pkg.BlstFr * 1)()
    # counts of zero: success, the pointers not looked at
    assert L.kzgamd_g1_mul_batch(None, None, None, 0, None) == 0
    assert L.kzgamd_g2_mul_batch(None, None, None, 0, None) == 0
    assert L.kzgamd_generate_trusted_setup(None, None, None, None, 0, 0, None, None) == 0
    # NULL arguments
    p1, p2 = (pkg.BlstP1 * 1)(), (pkg.BlstP2 * 1)()
    assert L.kzgamd_g1_mul_batch(None, None, one, 1, None) == -1 and L.kzgamd_g1_mul_batch(p1, None, None, 1, None) == -1
    assert L.kzgamd_g2_mul_batch(None, None, one, 1, None) == -1 and L.kzgamd_g2_mul_batch(p2, None, None, 1, None) == -1
    assert L.kzgamd_generate_trusted_setup(None, p1, None, None, 1, 0, None, None) == -1
    # the Lagrange form without a handle, or for a count that is no power of two
    assert L.kzgamd_generate_trusted_setup(None, None, p1, None, 1, 0, bytes(32), None) == 1
    # the tuning string: one key of these calls alone
    for bad in ("mul_slice=63", "mul_slice=32", "mul_slice=", "mul_slice=96", "spl=1", "mul_slice=64;spl=1", "mul_slices=64"):
        cfg = pkg.make_config(tuning=bad)
        assert L.kzgamd_g1_mul_batch(p1, None, one, 1, C.byref(cfg)) == -2, bad
        assert L.kzgamd_g2_mul_batch(p2, None, one, 1, C.byref(cfg)) == -2, bad
        assert L.kzgamd_generate_trusted_setup(None, p1, None, None, 1, 0, bytes(32), C.byref(cfg)) == -2, bad
    # a base at infinity: every output is infinity, whatever was there
    for arr, fn, base in ((( pkg.BlstP1 * 3)(), L.kzgamd_g1_mul_batch, pkg.BlstP1()), ((pkg.BlstP2 * 3)(), L.kzgamd_g2_mul_batch, pkg.BlstP2())):
        C.memset(arr, 0xa5, C.sizeof(arr))
        three = (pkg.BlstFr * 3)()
        assert fn(arr, C.byref(base), three, 3, None) == 0
        assert bytes(arr) == bytes(C.sizeof(arr))
    # a G1 base outside the subgroup: a point of order 3 of the curve
    x, y = E.torsion_point(3)
    mont = lambda v: (v << 384) % E.P
    low = pkg.BlstP1()
    C.memmove(C.byref(low), b"".join(mont(v).to_bytes(48, "little") for v in (x, y, 1)), 144)
    assert L.kzgamd_g1_mul_batch(p1, C.byref(low), one, 1, None) == 3
