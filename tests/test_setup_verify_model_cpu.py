"""tests/setup_verify_model.py pinned against itself and against Python's hashlib: the four checks of
kzgamd_verify_trusted_setup over discrete logarithms accept a setup built from a secret, name exactly the expected bits
for every tamper the GPU test applies, and the seed == NULL byte layout is the one include/kzg_mi355x.h spells out."""
import hashlib
import random

import pytest

import codec_model as CM
import fk20_model as M
import setup_model as S
import setup_verify_model as V

SIZES = [(4, 2), (8, 3)]
SEEDS = [bytes(32), b"\xff" * 32, bytes(range(32)), hashlib.sha256(b"setup_verify_model").digest()]


def setups(n1, n2, secret):
    w = M.root_of_order(n1)
    s = S.hash_to_bls_field(secret)
    return V.make_setup(s, n1, n2, w), w


@pytest.mark.parametrize("n1,n2", SIZES)
@pytest.mark.parametrize("secret", sorted(S.SECRETS))
def test_a_setup_built_from_a_secret_is_accepted(n1, n2, secret):
    (m, l, q), w = setups(n1, n2, S.SECRETS[secret])
    for seed in SEEDS:
        r = V.challenge(seed)
        assert 1 <= r < V.R
        assert V.failed_bits(m, l, q, r, w) == 0
        assert V.failed_bits(m, None, q, r) == 0


def test_the_challenge_is_hash_to_bls_field_and_never_zero():
    assert V.challenge(bytes(32)) == 1
    assert V.challenge(V.R.to_bytes(32, "big")) == 1
    assert V.challenge(b"\xff" * 32) == ((1 << 256) - 1) % V.R
    assert V.challenge((5).to_bytes(32, "big")) == 5


@pytest.mark.parametrize("n1,n2", SIZES)
def test_every_tamper_reports_exactly_its_bits(n1, n2):
    (m, l, q), w = setups(n1, n2, S.SECRETS["fk20"])
    other, _ = setups(n1, n2, hashlib.sha256(b"another secret").digest())
    table = V.tampers(n1, n2)
    assert len(table) >= 10
    for name, f in sorted(table.items()):
        tm, tl, tq = f(m, l, q, other)
        want = V.expected_bits(name, n1)
        for seed in SEEDS[1:]:
            r = V.challenge(seed)
            assert V.failed_bits(tm, tl, tq, r, w) == want, (name, n1, n2)
            if "L" not in name:
                assert V.failed_bits(tm, None, tq, r) == want & ~8, (name, n1, n2)
    # the secrets 1 and 0 are setups too: every point equal, every point after the first the identity
    for secret in ("one", "zero"):
        (m, l, q), w = setups(n1, n2, S.SECRETS[secret])
        assert V.failed_bits(m, l, q, V.challenge(SEEDS[2]), w) == 0
    assert m[1:] == [0] * (n1 - 1) and l == [pow(n1, V.R - 2, V.R)] * n1


def test_the_derived_seed_has_the_documented_layout():
    rnd = random.Random(19)
    g2 = [CM.compress(CM.mul(k, CM.G2)) for k in (1, 5, 25)]
    assert g2[0] == CM.G2_COMPRESSED
    for n1, n2 in SIZES:
        m_bytes, l_bytes = rnd.randbytes(48 * n1), rnd.randbytes(48 * n1)
        q_bytes = b"".join(g2[:n2])
        head = b"KZGAMD_VERIFY_SETUP_V1" + n1.to_bytes(8, "big") + n2.to_bytes(8, "big")
        assert len(head) == 22 + 16
        assert V.derive_seed(n1, n2, m_bytes, l_bytes, q_bytes) == hashlib.sha256(head + b"\x01" + m_bytes + l_bytes + q_bytes).digest()
        assert V.derive_seed(n1, n2, m_bytes, None, q_bytes) == hashlib.sha256(head + b"\x00" + m_bytes + q_bytes).digest()
        assert V.derive_seed(n1, n2, m_bytes, None, q_bytes) != V.derive_seed(n1, n2, m_bytes, l_bytes, q_bytes)
