"""kzgamd_pairings_verify_batch (pairing.hip: one wave per check on the GPU) through the C ABI, on both library flavours:
its verdicts must be kzgamd_pairings_verify's (the host code) item by item — for every count around the wave and slice
edges with true and false items in a seeded, non-periodic order, Jacobian inputs with Z = 1 and Z != 1, infinity on
either or both G1 sides, an identity G2 point on either side, a curve point outside G1, the reference's
verify_kzg_proof vectors as one batch, count = 0, the NULL-argument codes, and two threads calling at once."""
import ctypes as C
import random
import threading

import pytest

import g1_encodings as E
import oracle_ffi as O
from test_pairing_cpu import fr_mont, to_p1, unhex

pytestmark = pytest.mark.gpu

P = E.P
T_SCALAR = 0x1F2E3D4C5B6A79880123456789ABCDEF  # the batch's shared G2 point is [t]G2
POOL = 12


def p1_bytes(pt, z=1):
    """affine (x, y) or None -> the 144 bytes of a blst_p1 (Jacobian, Montgomery 2^384) with the given Z"""
    if pt is None:
        return bytes(144)
    vals = (pt[0] * z * z % P, pt[1] * z * z * z % P, z % P)
    return b"".join((v * (1 << 384) % P).to_bytes(48, "little") for v in vals)


def p1_array(kzg, blobs):
    return (kzg.BlstP1 * len(blobs)).from_buffer_copy(b"".join(blobs))


def host_verdicts(kzg, a1, a2, b1, b2, cache):
    out = []
    for a, b in zip(a1, b1):
        key = (a, b, bytes(a2), bytes(b2))
        if key not in cache:
            pa, pb = kzg.BlstP1.from_buffer_copy(a), kzg.BlstP1.from_buffer_copy(b)
            cache[key] = kzg.pairings_verify(pa, a2, pb, b2)
        out.append(cache[key])
    return out


@pytest.fixture(scope="module")
def pool():
    """[k]G, [k t]G and [k t + 1]G for a dozen k, affine: true and false partners for the shared G2 points [t]G2 and G2"""
    rnd = random.Random(77)
    ks = [1, 2, E.R - 1] + [rnd.randrange(1, E.R) for _ in range(POOL - 3)]
    return [(E.mul(k, E.G), E.mul(k * T_SCALAR % E.R, E.G), E.mul((k * T_SCALAR + 1) % E.R, E.G)) for k in ks]


@pytest.fixture(scope="module")
def host_cache():
    return {}


def draw(pool, rnd, n):
    """n items (a1 bytes, b1 bytes): true and false ones, Z = 1 and Z != 1, in a seeded order with no period"""
    a1, b1 = [], []
    for _ in range(n):
        pk, good, bad = pool[rnd.randrange(len(pool))]
        za, zb = (rnd.choice((1, 1, 7, 0xBEEF)) for _ in range(2))  # few values: the host's verdicts are cached by bytes
        a1.append(p1_bytes(pk, za))
        b1.append(p1_bytes(good if rnd.random() < 0.6 else bad, zb))
    return a1, b1


def test_every_count_around_the_wave_and_slice_edges(kzg, pool, host_cache):
    g2 = kzg.p2_generator()
    qt = kzg.p2_mult(g2, fr_mont(kzg, T_SCALAR))
    rnd = random.Random(5)
    slice_checks = kzg.pairing_info()
    for n in (1, 2, 3, 4, 5, 63, 64, 65, slice_checks + 1):
        a1, b1 = draw(pool, rnd, n)
        got = kzg.pairings_verify_batch(p1_array(kzg, a1), qt, p1_array(kzg, b1), g2)
        want = host_verdicts(kzg, a1, qt, b1, g2, host_cache)
        assert got == want, (n, [i for i in range(n) if got[i] != want[i]][:8])
        if n >= 5:
            assert any(want) and not all(want)


def test_infinity_identity_g2_and_a_point_outside_g1(kzg, pool, host_cache):
    g2, inf2 = kzg.p2_generator(), kzg.BlstP2()
    qt = kzg.p2_mult(g2, fr_mont(kzg, T_SCALAR))
    pk, good, bad = pool[3]
    outside = E.torsion_point(11)  # on the curve, of order 11: not in G1
    assert E.on_curve(outside) and E.mul(E.R, outside) is not None
    z = 0xBEEF
    items = [(None, good), (pk, None), (None, None), (pk, good), (pk, bad), (outside, good), (pk, outside), (outside, outside),
             (None, outside), (pool[1][0], pool[1][1])]
    a1 = [p1_bytes(a, z if i % 2 else 1) for i, (a, _) in enumerate(items)]
    b1 = [p1_bytes(b, 1 if i % 2 else z) for i, (_, b) in enumerate(items)]
    for a2, b2 in ((qt, g2), (inf2, g2), (qt, inf2), (inf2, inf2), (g2, g2)):
        got = kzg.pairings_verify_batch(p1_array(kzg, a1), a2, p1_array(kzg, b1), b2)
        assert got == host_verdicts(kzg, a1, a2, b1, b2, host_cache), (bytes(a2)[:4], bytes(b2)[:4], got)
    # what the rules say, not only what the host says: two skipped sides give true, one skipped side false
    got = kzg.pairings_verify_batch(p1_array(kzg, a1), qt, p1_array(kzg, b1), g2)
    assert got[:5] == [False, False, True, True, False]
    assert kzg.pairings_verify_batch(p1_array(kzg, a1), inf2, p1_array(kzg, b1), inf2) == [True] * len(items)


def test_the_reference_verify_kzg_proof_vectors_as_one_batch(kzg, golden, trusted_setup_text):
    """check_proof_single with the per-case G2 term moved to the G1 side, so that the batch shares its G2 points:
    e(C - [y]G + [z]proof, G2) == e(proof, [tau]G2); the verdicts are the vectors' expected outputs"""
    L = O.lib()
    toks = trusted_setup_text.split()
    tau_g2 = kzg.p2_uncompress(bytes.fromhex(toks[2 + 4096 + 1].decode()))
    g2 = kzg.p2_generator()
    a1, b1, want, refused = [], [], [], 0
    for case in golden["verify_kzg_proof"]:
        c, z, y, pr = (unhex(case[k]) for k in ("commitment", "z", "y", "proof"))
        ca, pa, zf, yf = O.G1Affine(), O.G1Affine(), O.Fr(), O.Fr()
        valid = len(c) == 48 and len(pr) == 48 and len(z) == 32 and len(y) == 32
        valid = valid and L.og1_uncompress(C.byref(ca), c) == 1 and L.og1_uncompress(C.byref(pa), pr) == 1
        valid = valid and L.ofr_from_be32(C.byref(zf), z) == 1 and L.ofr_from_be32(C.byref(yf), y) == 1
        cj, pj = O.G1(), O.G1()
        if valid:
            L.og1_from_affine(C.byref(cj), C.byref(ca))
            L.og1_from_affine(C.byref(pj), C.byref(pa))
            valid = (L.og1_is_inf(C.byref(cj)) or L.og1_in_subgroup(C.byref(cj))) and \
                    (L.og1_is_inf(C.byref(pj)) or L.og1_in_subgroup(C.byref(pj)))
        if not valid:
            assert case["output"] is None, case["name"]
            refused += 1
            continue
        g, yg, zp, lhs = O.G1(), O.G1(), O.G1(), O.G1()
        L.og1_generator(C.byref(g))
        L.og1_mul(C.byref(yg), C.byref(g), C.byref(yf))
        L.og1_neg(C.byref(yg), C.byref(yg))
        L.og1_add_or_dbl(C.byref(lhs), C.byref(cj), C.byref(yg))
        L.og1_mul(C.byref(zp), C.byref(pj), C.byref(zf))
        L.og1_add_or_dbl(C.byref(lhs), C.byref(lhs), C.byref(zp))
        a1.append(bytes(to_p1(kzg, lhs)))
        b1.append(bytes(to_p1(kzg, pj)))
        want.append(case["output"])
    assert len(want) + refused == 122 and sum(want) >= 30 and len(want) - sum(want) >= 30
    assert kzg.pairings_verify_batch(p1_array(kzg, a1), g2, p1_array(kzg, b1), tau_g2) == want


def test_count_zero_and_the_null_argument_codes(kzg, pool):
    L = kzg.lib()
    g2 = kzg.p2_generator()
    a = p1_array(kzg, [p1_bytes(pool[0][0])])
    ok = (C.c_bool * 1)(True)
    assert L.kzgamd_pairings_verify_batch(None, None, None, None, None, 0) == 0
    assert L.kzgamd_pairings_verify_batch(ok, a, C.byref(g2), a, C.byref(g2), 0) == 0 and ok[0] is True  # nothing written
    full = [ok, a, C.byref(g2), a, C.byref(g2)]
    for hole in range(5):
        args = list(full)
        args[hole] = None
        assert L.kzgamd_pairings_verify_batch(*args, 1) == -1, hole
    assert L.kzgamd_pairings_verify_batch(*full, 1) == 0 and ok[0] is True  # e(P, G2) == e(P, G2)
    assert kzg.pairings_verify_batch([], g2, [], g2) == []


def test_two_threads_with_different_g2_points(kzg, pool, host_cache):
    g2 = kzg.p2_generator()
    qt = kzg.p2_mult(g2, fr_mont(kzg, T_SCALAR))
    q5 = kzg.p2_mult(g2, fr_mont(kzg, 5))
    rnd = random.Random(9)
    a1, b1 = draw(pool, rnd, 70)
    # against ([5]G2, G2) the partners are wrong but for chance: item 0 is made a true one
    a5, b5 = list(a1), list(b1)
    a5[0], b5[0] = p1_bytes(E.mul(3, E.G)), p1_bytes(E.mul(15, E.G), 9)
    jobs = [(a1, qt, b1, g2), (a5, q5, b5, g2)]
    got, errors = [None, None], []

    def work(i):
        try:
            a, a2, b, b2 = jobs[i]
            for _ in range(3):
                got[i] = kzg.pairings_verify_batch(p1_array(kzg, a), a2, p1_array(kzg, b), b2)
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, (a, a2, b, b2) in enumerate(jobs):
        assert got[i] == host_verdicts(kzg, a, a2, b, b2, host_cache), i
    assert got[1][0] is True and any(got[0]) and not all(got[0])
