"""kzgamd_verify_trusted_setup / kzgamd_verify_trusted_setup_file through the C ABI, on both library flavours.

Valid setups come from kzgamd_generate_trusted_setup and from tests/golden/trusted_setup.txt and must pass, with and
without the Lagrange form, under explicit seeds and under seed == NULL.  Every tamper of tests/setup_verify_model.py is
applied to the points of a (64, 65) setup and must give return 1 with exactly the bits the model gives for the same
challenge (the model works on the logarithms, which the test knows: it made the setup)."""
import ctypes as C
import gzip
import hashlib
import os

import pytest

import setup_model as S
import setup_verify_model as V
from test_generate_setup_gpu import fr_bulk, fs_of, root

pytestmark = pytest.mark.gpu
R = S.R
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SECRET = hashlib.sha256(b"test_verify_setup_gpu").digest()
SEED = hashlib.sha256(b"a seed the maker did not know").digest()
_ref = {}


def setup_of(kzg, n1, n2, secret=SECRET):
    """(mono, lag, g2) as bytes lists, generated once per process"""
    key = ("setup", n1, n2, secret)
    if key not in _ref:
        mono, lag, g2 = kzg.generate_trusted_setup(n1, secret, num_g2=n2, fft_settings=fs_of(kzg))
        _ref[key] = ([bytes(mono[i]) for i in range(n1)], [bytes(lag[i]) for i in range(n1)], [bytes(g2[j]) for j in range(n2)])
    return _ref[key]


def arr(kzg, typ, raw):
    a = (typ * len(raw))()
    C.memmove(a, b"".join(raw), C.sizeof(a))
    return a


def verify(kzg, m, l, q, seed=SEED, config=None):
    return kzg.verify_trusted_setup(arr(kzg, kzg.BlstP1, m), arr(kzg, kzg.BlstP1, l) if l is not None else None, arr(kzg, kzg.BlstP2, q),
                                    len(m), len(q), fft_settings=fs_of(kzg) if l is not None else None, seed=seed, config=config)


@pytest.mark.parametrize("n1,n2", [(2, 2), (4, 2), (16, 3), (64, 65), (1024, 1024)])
def test_generated_setups_pass(kzg, n1, n2):
    m, l, q = setup_of(kzg, n1, n2)
    for seed in (SEED, None, bytes(32), b"\xff" * 32):
        assert verify(kzg, m, l, q, seed) == (0, 0), (n1, n2, seed)
        assert verify(kzg, m, None, q, seed) == (0, 0), (n1, n2, seed, "without L")


def test_a_small_slice_gives_the_same_verdict(kzg):
    m, l, q = setup_of(kzg, 64, 65)
    cfg = kzg.make_config(tuning="lincomb_slice=64")  # 64 terms of C and D: exactly one slice
    assert verify(kzg, m, l, q, config=cfg) == (0, 0)
    m, l, q = setup_of(kzg, 1024, 1024)  # 1023 terms: 16 slices, the last of 63
    assert verify(kzg, m, l, q, config=cfg) == (0, 0)
    bad = list(q)
    bad[1000] = q[999]
    assert verify(kzg, m, l, bad, config=cfg) == (1, 4)


def test_the_golden_setup_file_passes(kzg):
    path = os.path.join(GOLDEN, "trusted_setup.txt")
    assert kzg.verify_trusted_setup_file(path, fs_of(kzg), seed=SEED) == (0, 0)
    assert kzg.verify_trusted_setup_file(path, fs_of(kzg)) == (0, 0)


@pytest.mark.parametrize("secret", ["one", "zero"])
def test_degenerate_secrets_get_the_models_verdict(kzg, secret):
    """secret 1: every point is the generator; secret 0: every point after the first is the identity"""
    n1, n2 = 16, 3
    m, l, q = setup_of(kzg, n1, n2, S.SECRETS[secret])
    s = S.hash_to_bls_field(S.SECRETS[secret])
    w = root(fs_of(kzg), n1)
    mm, ml, mq = V.make_setup(s, n1, n2, w)
    want = V.failed_bits(mm, ml, mq, V.challenge(SEED), w)
    assert want == 0
    assert verify(kzg, m, l, q) == (1 if want else 0, want)
    assert verify(kzg, m, None, q, None) == (0, 0)
    if secret == "zero":
        assert m[1] == bytes(144) and q[1] == bytes(288)


def g1_of(kzg, v):
    return bytes(kzg.g1_mul_batch(fr_bulk(kzg, [v]), 1)[0])


def g2_of(kzg, v):
    return bytes(kzg.p2_mult(kzg.p2_generator(), fr_bulk(kzg, [v])[0]))


def test_every_tamper_reports_the_models_bits(kzg):
    n1, n2 = 64, 65
    m, l, q = setup_of(kzg, n1, n2)
    other_secret = hashlib.sha256(b"another secret").digest()
    s, s2 = S.hash_to_bls_field(SECRET), S.hash_to_bls_field(other_secret)
    w = root(fs_of(kzg), n1)
    model = V.make_setup(s, n1, n2, w)
    model2 = V.make_setup(s2, n1, n2, w)
    points2 = setup_of(kzg, n1, n2, other_secret)
    r = V.challenge(SEED)
    table = V.tampers(n1, n2)
    assert len(table) == 11
    for name, f in sorted(table.items()):
        tm, tl, tq = f(*model, model2)
        want = V.failed_bits(tm, tl, tq, r, w)
        assert want == V.expected_bits(name, n1) != 0, name
        # the same tamper on the points: every changed logarithm becomes the point of that logarithm
        pm = [m[i] if tm[i] == model[0][i] else g1_of(kzg, tm[i]) for i in range(n1)]
        pl = [l[i] if tl[i] == model[1][i] else g1_of(kzg, tl[i]) for i in range(n1)]
        pq = [q[j] if tq[j] == model[2][j] else (points2[2][j] if tq[j] == model2[2][j] else g2_of(kzg, tq[j])) for j in range(n2)]
        assert verify(kzg, pm, pl, pq) == (1, want), name
        if "L" not in name:
            assert verify(kzg, pm, None, pq) == ((1, want & ~8) if want & ~8 else (0, 0)), (name, "without L")
    # under seed == NULL the challenge is the library's own: the bits are those every challenge gives
    bad = list(m)
    bad[32] = m[31]
    assert verify(kzg, bad, l, q, None) == (1, 2 | 8)


def test_codes_2_and_3_and_null_pointers(kzg):
    L = kzg.lib()
    m, l, q = setup_of(kzg, 16, 3)
    am, al, aq = arr(kzg, kzg.BlstP1, m), arr(kzg, kzg.BlstP1, l), arr(kzg, kzg.BlstP2, q)
    fs = fs_of(kzg).handle
    failed = C.c_uint(77)
    assert L.kzgamd_verify_trusted_setup(fs, C.byref(failed), am, al, aq, 1, 3, SEED, None) == 2
    assert L.kzgamd_verify_trusted_setup(fs, C.byref(failed), am, al, aq, 16, 1, SEED, None) == 2
    assert L.kzgamd_verify_trusted_setup(fs, C.byref(failed), am, al, aq, 12, 3, SEED, None) == 3  # not a power of two
    assert L.kzgamd_verify_trusted_setup(None, C.byref(failed), am, al, aq, 16, 3, SEED, None) == 3  # L without a handle
    small = kzg.FFTSettings(3)
    assert L.kzgamd_verify_trusted_setup(small.handle, C.byref(failed), am, al, aq, 16, 3, SEED, None) == 3  # 16 > 8
    assert L.kzgamd_verify_trusted_setup(None, C.byref(failed), am, None, aq, 12, 3, SEED, None) == 0  # no L: any count, no handle
    assert failed.value == 0
    assert L.kzgamd_verify_trusted_setup(fs, C.byref(failed), None, al, aq, 16, 3, SEED, None) == -1
    assert L.kzgamd_verify_trusted_setup(fs, C.byref(failed), am, al, None, 16, 3, SEED, None) == -1
    assert L.kzgamd_verify_trusted_setup(fs, None, am, al, aq, 16, 3, SEED, None) == 0  # failed may be NULL
    assert L.kzgamd_verify_trusted_setup_file(fs, C.byref(failed), None, SEED, None) == -1
    for bad in ("lincomb_slice=63", "codec_slice=64", "spl=1"):
        cfg = kzg.make_config(tuning=bad)
        assert L.kzgamd_verify_trusted_setup(fs, C.byref(failed), am, al, aq, 16, 3, SEED, C.byref(cfg)) == -2, bad


def test_files_the_reader_refuses(kzg, tmp_path):
    def fixture(name):
        with gzip.open(os.path.join(GOLDEN, "setup_fixtures", name + ".txt.gz"), "rb") as f:
            return f.read()

    fs = fs_of(kzg)
    path = tmp_path / "setup.txt"
    path.write_bytes(fixture("invalid_chars"))
    assert kzg.verify_trusted_setup_file(str(path), fs, seed=SEED)[0] == 11
    # a valid fixture with one G1 line turned into an encoding no decoder accepts (infinity with the sign flag)
    tok = fixture("valid_short_hex").split()
    at = next(i for i, t in enumerate(tok) if i >= 2 and len(t) == 96)  # the first G1 point written as one token
    tok[at] = b"e0" + b"0" * 94
    path.write_bytes(b"\n".join(tok))
    assert kzg.verify_trusted_setup_file(str(path), fs, seed=SEED) == (13, 0)
