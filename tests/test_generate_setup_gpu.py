"""kzgamd_generate_trusted_setup (groupmul.hip) through the C ABI, on both library flavours: generate_trusted_setup of the
reference (blst/src/utils.rs:16-37) with the powers of the secret, both groups' multiplications and the Lagrange form
on the GPU.

Anchors, none of them the code under test:
  - the closed forms of tests/setup_model.py with the known secret: g1_monomial[i] = [s^i]G by the CPU oracle's og1_mul,
    g2_monomial[j] = [s^j]G2 by the host's kzgamd_p2_mult, g1_lagrange[i] = [L_i(s)]G;
  - the library's own fft_g1 (tested against the oracle elsewhere) on the monomial points;
  - bilinearity: e(g1[i + 1], G2) == e(g1[i], g2[1]) for a 4096-point setup, and the host pairing on three G2 powers;
  - a round trip through the c-kzg surface: the generated setup, compressed and loaded, commits a blob to [p(s)]G and
    proves and verifies it."""
import ctypes as C
import random

import pytest

import oracle_ffi as O
import setup_model as S

pytestmark = pytest.mark.gpu
R = S.R
_ref = {}
_fs = {}


def fs_of(kzg):
    """one FFTSettings of 4096 points per flavour"""
    if kzg.__name__ not in _fs:
        _fs[kzg.__name__] = kzg.FFTSettings(12)
    return _fs[kzg.__name__]


def fr_bulk(kzg, vals):
    raw = b"".join(((v << 256) % R).to_bytes(32, "little") for v in vals)
    arr = (kzg.BlstFr * max(len(vals), 1))()
    C.memmove(arr, raw, len(raw))
    return arr


def og1(p):
    g = O.G1()
    C.memmove(C.byref(g), bytes(p), 144)
    return g


def g1_of(v):
    """[v]G from the oracle, None for the identity; cached"""
    if ("g1", v) not in _ref:
        if v == 0:
            _ref[("g1", v)] = None
        else:
            L = O.lib()
            g, e = O.G1(), O.G1()
            L.og1_generator(C.byref(g))
            L.og1_mul(C.byref(e), C.byref(g), C.byref(O.fr_from_int(v)))
            _ref[("g1", v)] = e
    return _ref[("g1", v)]


def g2_of(kzg, v):
    """compressed [v]G2 from the host's double-and-add; cached"""
    if ("g2", v) not in _ref:
        _ref[("g2", v)] = kzg.p2_compress(kzg.p2_mult(kzg.p2_generator(), fr_bulk(kzg, [v])[0]))
    return _ref[("g2", v)]


def assert_g1(got, scalars, what):
    L = O.lib()
    for j, v in enumerate(scalars):
        g, e = og1(got[j]), g1_of(v)
        if e is None:
            assert L.og1_is_inf(C.byref(g)), (what, j, "expected the identity")
        else:
            assert not L.og1_is_inf(C.byref(g)) and L.og1_equal(C.byref(g), C.byref(e)), (what, j)


def assert_same_points(a, b, n, what):
    L = O.lib()
    for j in range(n):
        x, y = og1(a[j]), og1(b[j])
        ix, iy = L.og1_is_inf(C.byref(x)), L.og1_is_inf(C.byref(y))
        assert bool(ix) == bool(iy) and (ix or L.og1_equal(C.byref(x), C.byref(y))), (what, j)


def root(fs, order):
    """the handle's root of that order, out of Montgomery form"""
    r, _, _ = fs.roots()
    v = int.from_bytes(bytes(r[fs.max_width // order]), "little")
    return v * pow(1 << 256, R - 2, R) % R


@pytest.mark.parametrize("secret", sorted(S.SECRETS))
def test_small_setups_against_the_closed_forms(kzg, secret):
    fs = fs_of(kzg)
    s = S.hash_to_bls_field(S.SECRETS[secret])
    for num_g1 in (1, 2, 16, 64):
        pw = S.powers(s, num_g1)
        for num_g2 in sorted({0, 1, 2, num_g1}):
            mono, lag, g2 = kzg.generate_trusted_setup(num_g1, S.SECRETS[secret], num_g2=num_g2, fft_settings=fs)
            what = "%s %d %d" % (secret, num_g1, num_g2)
            assert_g1(mono, pw, what + " monomial")
            for j in range(num_g2):
                assert kzg.p2_compress(g2[j]) == g2_of(kzg, pow(s, j, R)), (what, "G2", j)
            assert_same_points(lag, fs.fft_g1(mono, num_g1, inverse=True), num_g1, what + " Lagrange against fft_g1")
            if num_g1 == 16:
                assert_g1(lag, S.lagrange_closed_form(s, 16, root(fs, 16)), what + " Lagrange closed form")
    # what the two degenerate secrets give
    mono, _, g2 = kzg.generate_trusted_setup(4, S.SECRETS[secret], num_g2=3, want_lagrange=False)
    if secret == "zero":
        assert_g1(mono, [1, 0, 0, 0], "secret zero")
        assert [bytes(g2[j]) == bytes(288) for j in range(3)] == [False, True, True]
    if secret == "one":
        assert_g1(mono, [1, 1, 1, 1], "secret one")
        assert all(kzg.p2_compress(g2[j]) == kzg.p2_compress(kzg.p2_generator()) for j in range(3))


def big_setup(kzg):
    key = ("big", kzg.__name__)
    if key not in _ref:
        _ref[key] = kzg.generate_trusted_setup(4096, S.SECRETS["fk20"], num_g2=65, fft_settings=fs_of(kzg))
    return _ref[key]


def test_pairing_consistency_of_a_4096_point_setup(kzg):
    mono, _, g2 = big_setup(kzg)
    gen2 = kzg.p2_generator()
    n = 4096
    a1 = (kzg.BlstP1 * (n - 1)).from_buffer_copy(bytes(mono)[144:])
    b1 = (kzg.BlstP1 * (n - 1)).from_buffer_copy(bytes(mono)[:144 * (n - 1)])
    ok = kzg.pairings_verify_batch(a1, gen2, b1, g2[1])  # e(g1[i + 1], G2) == e(g1[i], [s]G2)
    assert len(ok) == n - 1 and all(ok), [i for i, v in enumerate(ok) if not v][:8]
    gen1 = mono[0]
    for j in (1, 2, 64):
        assert kzg.pairings_verify(gen1, g2[j], mono[j], gen2), j
    assert not kzg.pairings_verify(gen1, g2[2], mono[3], gen2)


def poly_at_secret_from_blob(vals, s, w):
    """p(s) for the polynomial with p(w^brp(i)) = vals[i] (the blob's evaluation form), by the barycentric formula"""
    n = len(vals)
    bits = n.bit_length() - 1
    brp = lambda i: int(format(i, "0%db" % bits)[::-1], 2)
    acc = 0
    for i, v in enumerate(vals):
        wi = pow(w, brp(i), R)
        acc = (acc + v * wi % R * pow((s - wi) % R, R - 2, R)) % R
    return acc * (pow(s, n, R) - 1) % R * pow(n, R - 2, R) % R


def test_round_trip_through_the_ckzg_surface(kzg):
    mono, lag, g2 = big_setup(kzg)
    L = O.lib()
    buf = C.create_string_buffer(48)

    def compress_all(pts, n):
        out = []
        for j in range(n):
            g = og1(pts[j])
            L.og1_compress(buf, C.byref(g))
            out.append(buf.raw)
        return b"".join(out)

    g2_bytes = b"".join(kzg.p2_compress(g2[j]) for j in range(65))
    settings = kzg.KZGSettings.from_bytes(compress_all(mono, 4096), compress_all(lag, 4096), g2_bytes, kzg.make_config(no_tables=True))
    try:
        rnd = random.Random(4096)
        vals = [rnd.randrange(R) for _ in range(4096)]
        blob = b"".join(v.to_bytes(32, "big") for v in vals)
        s = S.hash_to_bls_field(S.SECRETS["fk20"])
        commitment = kzg.blob_to_kzg_commitment(blob, settings)
        e = g1_of(poly_at_secret_from_blob(vals, s, root(fs_of(kzg), 4096)))
        L.og1_compress(buf, C.byref(e))
        assert commitment == buf.raw, "the commitment is not [p(s)]G"
        proof = kzg.compute_blob_kzg_proof(blob, commitment, settings)
        assert kzg.verify_blob_kzg_proof(blob, commitment, proof, settings) is True
    finally:
        settings.close()


def test_generic_handle_over_a_generated_setup(kzg):
    fs = fs_of(kzg)
    secret = S.SECRETS["fk20"]
    s = S.hash_to_bls_field(secret)
    mono, _, g2 = kzg.generate_trusted_setup(64, secret, num_g2=2, want_lagrange=False)
    rnd = random.Random(64)
    coeffs = [rnd.randrange(R) for _ in range(64)]
    with kzg.PolyKZGSettings(fs, mono, 64, g2, 2) as ks:
        got = ks.commit(fr_bulk(kzg, coeffs), 64)
    assert_g1(got, [sum(c * pow(s, i, R) for i, c in enumerate(coeffs)) % R], "commit")


def test_errors_and_partial_outputs(kzg):
    fs = fs_of(kzg)
    L = kzg.lib()
    secret = S.SECRETS["fk20"]
    s = S.hash_to_bls_field(secret)
    p24, q24 = (kzg.BlstP1 * 24)(), (kzg.BlstP1 * 24)()
    assert L.kzgamd_generate_trusted_setup(fs.handle, p24, q24, None, 24, 0, secret, None) == 1
    assert L.kzgamd_generate_trusted_setup(None, p24, q24, None, 16, 0, secret, None) == 1
    assert L.kzgamd_generate_trusted_setup(fs.handle, None, None, None, 8192, 0, secret, None) == 0  # nothing wanted
    big = (kzg.BlstP1 * 8192)()
    assert L.kzgamd_generate_trusted_setup(fs.handle, None, big, None, 8192, 0, secret, None) == 2
    # the monomial points alone need neither a handle nor a power of two
    assert L.kzgamd_generate_trusted_setup(None, p24, None, None, 24, 0, secret, None) == 0
    assert_g1(p24, S.powers(s, 24), "24 monomial points")
    # any output left out: the others are what they are with all three
    n, n2 = 16, 5
    lag_want = S.lagrange_closed_form(s, n, root(fs, n))
    for want_mono, want_lag, want_g2 in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        mono, lag, g2 = (kzg.BlstP1 * n)(), (kzg.BlstP1 * n)(), (kzg.BlstP2 * n2)()
        for b in (mono, lag, g2):
            C.memset(b, 0x3c, C.sizeof(b))
        rc = L.kzgamd_generate_trusted_setup(fs.handle, mono if want_mono else None, lag if want_lag else None,
                                             g2 if want_g2 else None, n, n2, secret, None)
        assert rc == 0, (want_mono, want_lag, want_g2)
        if want_mono:
            assert_g1(mono, S.powers(s, n), "monomial alone")
        if want_lag:
            assert_g1(lag, lag_want, "Lagrange alone")
        if want_g2:
            assert all(kzg.p2_compress(g2[j]) == g2_of(kzg, pow(s, j, R)) for j in range(n2))
    # both counts zero: nothing is touched
    mono, g2 = (kzg.BlstP1 * 1)(), (kzg.BlstP2 * 1)()
    C.memset(mono, 0x3c, 144)
    C.memset(g2, 0x3c, 288)
    assert L.kzgamd_generate_trusted_setup(fs.handle, mono, mono, g2, 0, 0, secret, None) == 0
    assert bytes(mono) == b"\x3c" * 144 and bytes(g2) == b"\x3c" * 288
    # slices: a setup cut into pieces of 64 outputs is the same setup
    cfg = kzg.make_config(tuning="mul_slice=64")
    a = kzg.generate_trusted_setup(256, secret, num_g2=130, fft_settings=fs, config=cfg)
    b = kzg.generate_trusted_setup(256, secret, num_g2=130, fft_settings=fs)
    assert_same_points(a[0], b[0], 256, "sliced monomial")
    assert_same_points(a[1], b[1], 256, "sliced Lagrange")
    assert bytes(a[2]) == bytes(b[2])
    assert_g1([a[0][255]], [pow(s, 255, R)], "the last sliced power")
