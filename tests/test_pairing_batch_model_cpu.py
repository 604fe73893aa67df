"""The Python-integer model of the device pairing (tests/pairing_model.py) pinned to the product's host code on the CPU,
no GPU involved: the model follows fp12w.hip.h formula for formula, and its verdicts must be kzgamd_pairings_verify's
(host_pairing.h) on bilinearity cases, the same cases off by one, infinity on either or both G1 sides and the
reference's verify_kzg_proof vectors.  The GPU modules then hold the device to the model, value for value.

Also here: the case generator of the device harness keeps the bounds the header documents, the harness cross-compiles
for gfx950, and the header, the library, the Python module and the Rust sys crate name the new entry points."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

import lane_harness as H
import oracle_ffi as O
import pairing_model as M
from test_pairing_cpu import fr_mont, g1_mul_gen, to_p1, unhex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "device_checks", "pairing_check.hip")
NAMES = ("kzgamd_pairings_verify_batch", "kzgamd_pairing_info")

_tables = {}


def p1_words(p):
    return list(struct.unpack("<36I", bytes(p)))


def table_of(q):
    """the model's Montgomery line table of a BlstP2 (None for the identity), cached by the point's bytes"""
    key = bytes(q)
    if key not in _tables:
        _tables[key] = M.table_mont(M.g2_line_table(M.g2_affine_from_jacobian_mont384(struct.unpack("<72I", key))))
    return _tables[key]


def model_verdict(a1, a2, b1, b2):
    return M.pairing_check(p1_words(a1), p1_words(b1), [table_of(a2), table_of(b2)])[0]


def test_the_model_is_the_host_code_on_bilinearity_and_infinity(kzg):
    L = O.lib()
    g2 = kzg.p2_generator()
    rng = random.Random(2)
    pairs = [(1, 1), (2, 3), (5, 7), (O.R - 1, 2), (3, O.R - 1)] + [(rng.randrange(1, O.R), rng.randrange(1, O.R)) for _ in range(7)]
    assert len(pairs) >= 12
    for k, t in pairs:
        pk, pkt, off = (to_p1(kzg, g1_mul_gen(L, v)) for v in (k, k * t, k * t + 1))
        qt = kzg.p2_mult(g2, fr_mont(kzg, t))
        assert model_verdict(pk, qt, pkt, g2) is True and kzg.pairings_verify(pk, qt, pkt, g2)
        assert model_verdict(pkt, g2, pk, qt) is True and kzg.pairings_verify(pkt, g2, pk, qt)
        # one side off by one
        assert model_verdict(pk, qt, off, g2) is False and not kzg.pairings_verify(pk, qt, off, g2)
        assert model_verdict(off, g2, pk, qt) is False and not kzg.pairings_verify(off, g2, pk, qt)
    p1, inf1, inf2 = to_p1(kzg, g1_mul_gen(L, 1)), kzg.BlstP1(), kzg.BlstP2()
    for a1, a2, b1, b2 in ((inf1, g2, p1, g2), (p1, g2, inf1, g2), (inf1, g2, inf1, g2), (inf1, g2, p1, inf2),
                           (p1, inf2, p1, inf2), (p1, inf2, p1, g2)):
        assert model_verdict(a1, a2, b1, b2) == kzg.pairings_verify(a1, a2, b1, b2)
    assert model_verdict(inf1, g2, inf1, g2) is True and model_verdict(inf1, g2, p1, g2) is False


def test_the_model_is_the_host_code_on_the_reference_vectors(kzg, golden, trusted_setup_text):
    """check_proof_single as tests/test_pairing_cpu.py rebuilds it: e(C - [y]G, G2) == e(proof, [tau]G2 - [z]G2)"""
    L = O.lib()
    toks = trusted_setup_text.split()
    tau_g2 = kzg.p2_uncompress(bytes.fromhex(toks[2 + 4096 + 1].decode()))
    g2 = kzg.p2_generator()
    seen = {True: 0, False: 0}
    for case in golden["verify_kzg_proof"]:
        c, z, y, pr = (unhex(case[k]) for k in ("commitment", "z", "y", "proof"))
        ca, pa, zf, yf = O.G1Affine(), O.G1Affine(), O.Fr(), O.Fr()
        if not (len(c) == 48 and len(pr) == 48 and len(z) == 32 and len(y) == 32):
            continue
        if not (L.og1_uncompress(C.byref(ca), c) == 1 and L.og1_uncompress(C.byref(pa), pr) == 1 and
                L.ofr_from_be32(C.byref(zf), z) == 1 and L.ofr_from_be32(C.byref(yf), y) == 1):
            continue
        cj, pj, g, yg, cmy = O.G1(), O.G1(), O.G1(), O.G1(), O.G1()
        L.og1_from_affine(C.byref(cj), C.byref(ca))
        L.og1_from_affine(C.byref(pj), C.byref(pa))
        if not ((L.og1_is_inf(C.byref(cj)) or L.og1_in_subgroup(C.byref(cj))) and (L.og1_is_inf(C.byref(pj)) or L.og1_in_subgroup(C.byref(pj)))):
            continue
        L.og1_generator(C.byref(g))
        L.og1_mul(C.byref(yg), C.byref(g), C.byref(yf))
        L.og1_neg(C.byref(yg), C.byref(yg))
        L.og1_add_or_dbl(C.byref(cmy), C.byref(cj), C.byref(yg))
        zneg, zero, zm = O.Fr(), O.fr_from_int(0), kzg.BlstFr()
        L.ofr_sub(C.byref(zneg), C.byref(zero), C.byref(zf))
        C.memmove(C.byref(zm), C.byref(zneg), 32)
        s_minus_z = kzg.p2_add(tau_g2, kzg.p2_mult(g2, zm))
        want = kzg.pairings_verify(to_p1(kzg, cmy), g2, to_p1(kzg, pj), s_minus_z)
        assert want == case["output"], case["name"]
        if seen[want] >= 14:
            continue
        assert model_verdict(to_p1(kzg, cmy), g2, to_p1(kzg, pj), s_minus_z) is want, case["name"]
        seen[want] += 1
    assert seen[True] >= 10 and seen[False] >= 10 and seen[True] + seen[False] >= 20, seen


def test_the_frobenius_constants_and_the_generator_are_the_host_codes(kzg):
    """g[1]^6 = xi^(p-1) and the model's G2 generator is the library's"""
    one = M.RW
    g1 = tuple(v * pow(M.RW, -1, M.P) % M.P for v in M.FROB[1])
    acc = (1, 0)
    for _ in range(6):
        acc = M.g2f_mul(acc, g1)
    xi_p = (1, M.P - 1)  # (1 + u)^p = 1 - u
    assert M.g2f_mul(acc, (1, 1)) == xi_p and M.FROB[0] == (one, 0)
    assert M.g2_affine_from_jacobian_mont384(struct.unpack("<72I", bytes(kzg.p2_generator()))) == M.G2_GEN


def test_the_case_generator_keeps_the_documented_bounds():
    """every unit case is built from operands at the bounds fp12w.hip.h states — R-form operands up to 2p - 1 in limb
    forms with limbs at 2^28, line coefficients up to 8p — and the model's own assertions (subtrahends under their pads,
    Fp2 products inside the 2p product bound, R-form results) hold on all of them"""
    cases = M.unit_cases(random.Random(11), per_op=6)
    by_op = {}
    for c in cases:
        by_op.setdefault(c.op, []).append(c)
        assert len(c.words) == M.UNIT_NIN and all(0 <= w < 1 << 32 for w in c.words)
        for k in range(M.UNIT_PROG + 2, M.UNIT_NIN, 16):
            limbs = c.words[k:k + 16]
            assert all(w <= M.LIMB for w in limbs[:13]) and limbs[14] == 0 and limbs[15] == 0, c.tag
        assert all(v < 2 * M.P for v in c.expect), c.tag
    assert set(by_op) == {M.OP_MUL, M.OP_SQR, M.OP_CSQR, M.OP_CONJ, M.OP_FROB, M.OP_INV, M.OP_LINE}
    assert any(M.LIMB in c.words[M.UNIT_PROG + 2:] for c in cases), "no operand with a limb at 2^28"
    # a subtrahend above its pad is refused, not wrapped
    with pytest.raises(AssertionError):
        M.subk(8, 0, 8 * M.P)
    # the program is the one pairing.hip builds: same length, the line steps in order
    prog = M.FULL_PROGRAM
    steps = [w >> 24 for w in prog if w & 255 == M.OP_LINE]
    assert steps == list(range(M.LINE_STEPS)) and len(prog) <= M.PAIRING_PROG and prog[-1] == 0


def test_the_device_harness_cross_compiles_for_gfx950(tmp_path):
    out = str(tmp_path / "pairing_check")
    p = subprocess.run(H.compile_command(out, [], SOURCE), capture_output=True, text=True)
    assert p.returncode == 0 and os.path.exists(out), p.stderr[-3000:]


def test_header_library_python_module_and_rust_sys_crate_name_the_entry_points():
    from conftest import load_package
    from test_host_cpu import _c_prototypes, _rust_externs

    protos = _c_prototypes()
    ext = _rust_externs(os.path.join(ROOT, "rust-kzg_amd", "rust", "src", "lib.rs"))
    pkg = load_package("product")
    L = pkg.lib()
    for name, nargs in zip(NAMES, (6, 1)):
        assert len(protos[name]) == nargs, (name, protos[name])
        assert len(ext[name]) == nargs, (name, ext[name])
        assert name in pkg.EXPORTS and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert callable(pkg.pairings_verify_batch) and callable(pkg.pairing_info)
    # host-only answers: the slice size, count = 0 with no pointer looked at, the NULL-argument code
    assert 64 <= pkg.pairing_info() <= 1 << 20
    assert L.kzgamd_pairings_verify_batch(None, None, None, None, None, 0) == 0
    g2 = pkg.p2_generator()
    assert L.kzgamd_pairings_verify_batch(None, C.byref(pkg.BlstP1()), C.byref(g2), C.byref(pkg.BlstP1()), C.byref(g2), 1) == -1
