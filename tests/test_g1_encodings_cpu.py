"""tests/g1_encodings.py — the catalogue of crafted G1 encodings the GPU decode / subgroup-check tests are built on — is
held here, without a GPU, to three implementations that share no code with it or with each other: the oracle, the host
code of the library (csrc/host_g1.h) and the device code compiled for the host (csrc/g1_io.hip.h: g1io::uncompress and
the single-lane membership test affpt_in_g1)."""
import ctypes as C
import subprocess

import pytest

import g1_encodings as E
from test_host_cpu import build_g1check, build_g1io


def _run(exe, encodings):
    out = subprocess.run([str(exe)], input="\n".join(b.hex() for b in encodings) + "\n", capture_output=True, text=True,
                         check=True).stdout.split("\n")
    return [ln for ln in out if ln and not ln.startswith("c ")]


def test_the_catalogue_holds_what_it_promises():
    cat = E.catalogue()
    assert all(len(b) == 48 and cls in (0, 1, 2) for _, b, cls in cat)
    valid, outside, invalid = E.by_class(0), E.by_class(2), E.by_class(1)
    signs = [b[0] >> 5 & 1 for _, b in valid if not b[0] & 0x40]
    assert signs.count(0) >= 8 and signs.count(1) >= 8
    assert len(outside) >= 27 and len(invalid) >= 20
    names = {name for name, _, _ in cat}
    for q in E.COFACTOR_PRIMES:
        for form in ("order %d", "order %d, negated", "order %d + G"):
            assert form % q in names
        t = E.decode(next(b for name, b in outside if name == "order %d" % q))
        assert t is not None and E.on_curve(t) and E.mul(q, t) is None      # exact order q: q is prime
        assert E.mul(E.BLS_X, t) == E.neg(t) and E.mul(E.BLS_X ** 2, t) == t  # what the endomorphism test's chain meets
        tg = E.decode(next(b for name, b in outside if name == "order %d + G" % q))
        assert E.mul(E.R, tg) == E.mul(E.R % q, t) != None and E.mul(q, tg) == E.mul(q, E.G)  # noqa: E711
    assert E.decode(dict(outside)["(0, 2)"]) == (0, 2) and E.decode(dict(outside)["(0, -2)"]) == (0, E.P - 2)
    # the classes of the flag table: compressed points and the one infinity are all that decodes
    for name, b, cls in cat:
        if name.startswith("flags "):
            assert (cls != 1) == (name[6:9] in ("100", "101") or name == "flags 110 over zero"), name
    assert E.on_curve(E.G) and E.mul(E.R, E.G) is None


def test_the_oracle_classifies_the_catalogue_alike(oracle):
    import oracle_ffi as O

    L = oracle.lib()
    for name, b, cls in E.catalogue():
        a, p = O.G1Affine(), O.G1()
        if not L.og1_uncompress(C.byref(a), b):
            assert cls == 1, name
            continue
        if not b[0] & 0x40:
            L.og1_from_affine(C.byref(p), C.byref(a))
            want = E.decode(b)
            assert (O.fp_to_int(a.x), O.fp_to_int(a.y)) == want, name  # the sign of y included
        assert cls == (0 if L.og1_in_subgroup(C.byref(p)) else 2), name
        buf = C.create_string_buffer(48)
        L.og1_compress(buf, C.byref(p))
        assert buf.raw == b == E.compress(E.decode(b)), name


@pytest.mark.parametrize("code", ["host_g1.h", "g1_io.hip.h"])
def test_host_and_device_code_classify_the_catalogue_alike(tmp_path, code):
    """host_p1_uncompress + host_p1_in_g1, and g1io::uncompress + affpt_in_g1 (what k_decode_check_g1<true> and
    k_check_commitments run per lane) compiled for the host: the catalogue's class for every entry, and every entry that
    decodes compresses back to itself."""
    cat = E.catalogue()
    lines = _run(build_g1check(tmp_path) if code == "host_g1.h" else build_g1io(tmp_path), [b for _, b, _ in cat])
    assert len(lines) == len(cat)
    seen = {0: 0, 1: 0, 2: 0}
    for (name, b, cls), ln in zip(cat, lines):
        if ln == "bad":
            got = 1
        else:
            f = ln.split()
            in_g1, again = (f[1], f[2]) if code == "host_g1.h" else (f[3], f[1])
            got = 0 if int(in_g1) else 2
            assert again == b.hex(), name
        assert got == cls, (name, b.hex(), ln)
        seen[got] += 1
    assert seen[0] >= 35 and seen[1] >= 20 and seen[2] >= 27
