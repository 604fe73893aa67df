"""Every form of the guard in front of the c-kzg surface — decode 48 bytes, test membership in G1 — on the crafted
encodings of tests/g1_encodings.py (every class derived there with Python integers and pinned on the oracle, host_g1.h
and the host-compiled g1_io.hip.h by tests/test_g1_encodings_cpu.py).  The MSMs behind the guard are created G1_TRUSTED,
so a form that lets a torsion point through, picks the wrong root, or writes a status to the wrong row is a soundness
bug that neither random data nor the reference's vectors show.

  form                                          reached here through
  host_g1.h                                     proof batch, n = 6 and n = 64 (n <= host_check_max)
  k_decode_g1_wide + k_affpts_in_g1_wide        verification np <= 4096; proof batch host_check_max=0, n <= 512; n = 65, 512
  k_decode_check_g1<true> (single lane)         verification with wide_check=0, and np = 4097 by size
  k_check_commitments (single lane)             proof batch host_check_max=0;wide_check=0, and n = 513 by size

Seam A is kzgamd_verify_kzg_proof_batch_g1 (no blobs; it says which of proof / commitment / encoding failed and returns
the two sums the oracle restates); seam B the commitments of kzgamd_compute_blob_kzg_proof_batch (only hashed and
validated).  All comparisons are exact.  The error texts are read from stderr under KZGAMD_DEBUG."""
import ctypes as C
import gzip
import json
import os
import random
import time

import pytest

import g1_encodings as E
import oracle_ffi as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SETUP = os.path.join(GOLDEN, "trusted_setup.txt")
BLOB = 131072


def distinct(cls):
    """the catalogue's entries of a class, one per byte string (the flag table repeats some)"""
    seen, out = set(), []
    for name, b in E.by_class(cls):
        if b not in seen:
            seen.add(b)
            out.append((name, b))
    return out


VALID = [b for _, b in E.by_class(0)]          # all 37, repeats included
BAD = [(name, b, 1) for name, b in distinct(1)] + [(name, b, 2) for name, b in distinct(2)]
PROBE = dict(E.by_class(2))
EDGE_PROBES = [(name, PROBE[name]) for name in ("(0, 2)", "order 11", "order 52437899 + G")]


@pytest.fixture(scope="module")
def forms(kzg):
    """default keys / the wide kernels for the commitments of small proof batches / single lane everywhere; 1 GB tables,
    so that three objects load quickly and sit side by side"""
    made = {}
    try:
        for name, tuning in (("default", None), ("wide", "host_check_max=0"), ("lane", "host_check_max=0;wide_check=0")):
            made[name] = kzg.KZGSettings.from_file(SETUP, kzg.make_config(table_budget_gb=1, tuning=tuning))
        yield made
    finally:
        for s in made.values():
            s.close()


@pytest.fixture
def texts(monkeypatch, capfd):
    """why a call returned C_KZG_BADARGS: the library says it on stderr under KZGAMD_DEBUG"""
    monkeypatch.setenv("KZGAMD_DEBUG", "1")

    def refused(kzg, call, text):
        capfd.readouterr()
        with pytest.raises(kzg.KzgAmdError) as e:
            call()
        assert str(e.value).endswith("C_KZG_RET %d" % kzg.C_KZG_BADARGS)
        said = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("kzg_mi355x:")]
        assert said == ["kzg_mi355x: " + text], said

    return refused


# ---------------------------------------------------------------- seam A: verify_kzg_proof_batch_g1
_scalars = {}
_oracle_sums = {}


def scalars(n):
    if n not in _scalars:
        rnd = random.Random(4844 + n)
        _scalars[n] = (b"".join(rnd.randrange(O.R).to_bytes(32, "big") for _ in range(n)),
                       b"".join(rnd.randrange(O.R).to_bytes(32, "big") for _ in range(n)))
    return _scalars[n]


def valid_batch(n):
    """n valid proofs and, rotated by one, n valid commitments (infinity among them), with seeded z and y"""
    ps = b"".join(VALID[i % len(VALID)] for i in range(n))
    cs = b"".join(VALID[(i + 1) % len(VALID)] for i in range(n))
    return (cs,) + scalars(n) + (ps,)


def oracle_sums(n):
    """the oracle's (proof_lincomb, rhs) of valid_batch(n), compressed; computed once for both library flavours"""
    if n not in _oracle_sums:
        cs, zs, ys, ps = valid_batch(n)
        a, b = O.G1(), O.G1()
        t0 = time.perf_counter()
        assert O.lib().overify_kzg_proof_batch_g1(C.byref(a), C.byref(b), cs, zs, ys, ps, n) == 0
        if n > 1000:
            print("oracle, verify_kzg_proof_batch up to the pairing, n = %d: %.2f s" % (n, time.perf_counter() - t0))
        _oracle_sums[n] = (a, b)
    return _oracle_sums[n]


def accepts(kzg, s, n):
    cs, zs, ys, ps = valid_batch(n)
    got = kzg.verify_kzg_proof_batch_g1(cs, zs, ys, ps, n, s)
    for g, want in zip(got, oracle_sums(n)):
        p = O.G1()
        C.memmove(C.byref(p), C.byref(g), 144)
        assert O.lib().og1_equal(C.byref(p), C.byref(want)) == 1, n


def with_probe(batch, n, role, pos, probe):
    cs, zs, ys, ps = batch
    if role == "proof":
        ps = ps[:48 * pos] + probe + ps[48 * (pos + 1):]
    else:
        cs = cs[:48 * pos] + probe + cs[48 * (pos + 1):]
    assert len(ps) == len(cs) == 48 * n
    return cs, zs, ys, ps


def said_for(cls, role):
    return "Invalid G1 encoding" if cls == 1 else "Invalid proof" if role == "proof" else "Invalid commitment"


@pytest.mark.parametrize("form", ["default", "lane"])
def test_verification_accepts_every_valid_entry_with_the_oracles_sums(kzg, forms, form):
    """All cls 0 entries as proofs and, rotated by one, as commitments (np = 75: the last wave of k_decode_g1_wide holds
    three points): a wrong root, or an infinity that contributes something, changes the sums.  Then n = 1 .. 5, np = 3,
    5, 7, 9, 11, so that the last wave holds 3, 1, 3, 1, 3 points."""
    assert sum(1 for b in VALID if b[0] & 0x20) >= 8 and VALID[0][0] == 0xC0
    for n in (len(VALID), 1, 2, 3, 4, 5):
        accepts(kzg, forms[form], n)


@pytest.mark.parametrize("role", ["proof", "commitment"])
@pytest.mark.parametrize("form", ["default", "lane"])
def test_verification_refuses_every_bad_entry_and_says_why(kzg, forms, texts, form, role):
    """Each cls 1 and cls 2 entry alone in an otherwise valid batch of 6 (np = 13: positions 0 .. 5 are the four rows of
    the first wave and two of the second as a proof, and rows 2 .. 3 | 0 .. 3 of waves 1 .. 2 as a commitment); after
    each refusal the valid batch gives the oracle's sums again: d_vstat, d_vpts and the MSM object are reused."""
    s, n = forms[form], 6
    batch = valid_batch(n)
    accepts(kzg, s, n)
    assert len(BAD) >= 45
    for i, (name, probe, cls) in enumerate(BAD):
        cs, zs, ys, ps = with_probe(batch, n, role, i % n, probe)
        texts(kzg, lambda: kzg.verify_kzg_proof_batch_g1(cs, zs, ys, ps, n, s), said_for(cls, role))
        accepts(kzg, s, n)


@pytest.mark.parametrize("n", [2047, 2048])
def test_verification_by_size_on_either_side_of_the_wide_limit(kzg, forms, texts, n):
    """np = 2n + 1 = 4095 is the last size of the wide kernels, 4097 the first of k_decode_check_g1<true>: a (0, 2) proof
    and a torsion + G commitment at the ends and at the 64-lane block edge are refused, the valid batch gives the
    oracle's sums (one oracle call per size, ~2.3 s on a host core, shared by both flavours)."""
    s = forms["default"]
    batch = valid_batch(n)
    accepts(kzg, s, n)
    for pos in (0, 63, 64, n - 1):
        for role, probe in (("proof", PROBE["(0, 2)"]), ("commitment", PROBE["order 10177 + G"])):
            cs, zs, ys, ps = with_probe(batch, n, role, pos, probe)
            texts(kzg, lambda: kzg.verify_kzg_proof_batch_g1(cs, zs, ys, ps, n, s), said_for(2, role))
    accepts(kzg, s, n)


# ---------------------------------------------------------------- seam B: the commitments of a proof batch
_oracle_proofs = {}


@pytest.fixture(scope="module")
def triples(golden, blob_loader):
    """(blob, its commitment, its proof) of the reference's compute_blob_kzg_proof vectors"""
    out = [(blob_loader(c["blob"]), bytes.fromhex(c["commitment"][2:]), bytes.fromhex(c["output"][2:]))
           for c in golden["compute_blob_kzg_proof"] if c["output"] is not None]
    assert len(out) == 7
    return out


def oracle_proof(oracle_settings, blob, commitment):
    """ocompute_blob_kzg_proof for a commitment that need not belong to the blob: it only enters the challenge"""
    key = (hash(blob), commitment)
    if key not in _oracle_proofs:
        out = C.create_string_buffer(48)
        assert O.lib().ocompute_blob_kzg_proof(out, blob, commitment, C.byref(oracle_settings)) == 0
        _oracle_proofs[key] = out.raw
    return _oracle_proofs[key]


def proof_batch(triples, n, pos, commitment):
    """n blobs with their own commitments, except that blob `pos` comes with `commitment`"""
    pick = [triples[k % len(triples)] for k in range(n)]
    blobs = b"".join(t[0] for t in pick)
    cs = b"".join(commitment if k == pos else t[1] for k, t in enumerate(pick))
    return blobs, cs, [t[2] for t in pick]


SMALL = {"wide": (1, 3, 4, 5, 9), "lane": (1, 3, 4, 5, 9), "default": (6,)}  # default: n <= 64 is the host form


@pytest.mark.parametrize("form", ["default", "wide", "lane"])
def test_proof_batch_accepts_every_valid_commitment(kzg, forms, triples, oracle_settings, form):
    """A cls 0 commitment — infinity included — that does not belong to its blob is still a valid argument: the proof is
    the oracle's for that (blob, commitment), the other proofs of the batch are the vectors'."""
    s, sizes = forms[form], SMALL[form]
    for i, (name, c) in enumerate(distinct(0)):
        n = sizes[i % len(sizes)]
        pos = i % n
        blobs, cs, want = proof_batch(triples, n, pos, c)
        want[pos] = oracle_proof(oracle_settings, blobs[BLOB * pos:BLOB * (pos + 1)], c)
        assert kzg.compute_blob_kzg_proof_batch(blobs, cs, n, s) == want, name


@pytest.mark.parametrize("form", ["default", "wide", "lane"])
def test_proof_batch_refuses_every_bad_commitment(kzg, forms, texts, triples, form):
    """Each cls 1 and cls 2 entry, one call each, at a position that moves through the rows of a wave and into the
    second and third wave (n = 9); then the batch with its own commitments gives the vectors' proofs."""
    s, sizes = forms[form], SMALL[form]
    for i, (name, probe, cls) in enumerate(BAD):
        n = sizes[i % len(sizes)]
        blobs, cs, _ = proof_batch(triples, n, i % n, probe)
        texts(kzg, lambda: kzg.compute_blob_kzg_proof_batch(blobs, cs, n, s), "Invalid commitment")
    for n in sizes:
        blobs, cs, want = proof_batch(triples, n, -1, None)
        assert kzg.compute_blob_kzg_proof_batch(blobs, cs, n, s) == want


@pytest.mark.parametrize("n", [64, 65, 512, 513])
def test_proof_batch_by_size_at_the_edges_of_each_form(kzg, forms, texts, triples, n):
    """Default keys: 64 commitments are the last the host checks, 65 .. 512 go through the wide kernels (d_cpts holds
    512), 513 is the first batch of k_check_commitments.  One blob repeated; (0, 2), a point of order 11 and a torsion
    + G at the ends and at the 64-lane block edges."""
    s = forms["default"]
    blob, c, proof = triples[1]
    blobs = blob * n
    for pos in sorted({0, 63, 64, 511, 512, n - 1}):
        if pos >= n:
            continue
        for name, probe in EDGE_PROBES:
            cs = c * pos + probe + c * (n - 1 - pos)
            texts(kzg, lambda: kzg.compute_blob_kzg_proof_batch(blobs, cs, n, s), "Invalid commitment")
    assert kzg.compute_blob_kzg_proof_batch(blobs, c * n, n, s) == [proof] * n


# ---------------------------------------------------------------- the reference's vectors with single-lane checks
@pytest.fixture(scope="module")
def vec():
    with open(os.path.join(GOLDEN, "kzg_mainnet_7594.json")) as f:
        v = json.load(f)
    with gzip.open(os.path.join(GOLDEN, v["cells_file"]), "rb") as f:
        blob = f.read()
    v["_cells"] = [blob[i: i + 2048] for i in range(0, len(blob), 2048)]
    return v


def test_blob_batch_verification_vectors_with_single_lane_checks(kzg, forms, golden, blob_loader):
    """tests/test_verify_gpu.py's replay of verify_blob_kzg_proof_batch, expectations included, on wide_check=0"""
    import test_verify_gpu as V

    V.test_vectors_verify_blob_kzg_proof_batch(kzg, forms["lane"], golden, blob_loader)


def test_cell_batch_verification_vectors_with_single_lane_checks(kzg, forms, vec):
    """tests/test_cells7594_gpu.py's replay of verify_cell_kzg_proof_batch, expectations included, on wide_check=0"""
    import test_cells7594_gpu as C7

    C7.test_vectors_verify_cell_kzg_proof_batch(kzg, vec, forms["lane"])


@pytest.mark.parametrize("form", ["default", "lane"])
def test_cell_batch_refuses_low_order_points(kzg, forms, texts, vec, form):
    """decode_points of ckzg_7594.hip (proofs | distinct commitments | the 64 monomial points of the first call): a
    valid vector verifies, and raises with its first proof replaced by (0, 2) or its first commitment by a point of
    order 11."""
    import test_cells7594_gpu as C7

    s = forms[form]
    case = next(c for c in vec["verify_cell_kzg_proof_batch"] if c["output"] is True and len(c["cell_indices"]) >= 4)
    cells, ok = C7.cell_bytes(vec, case["cells"])
    assert ok
    coms = b"".join(C7.unhex(c) for c in case["commitments"])
    prfs = b"".join(C7.unhex(p) for p in case["proofs"])
    idx = case["cell_indices"]
    assert kzg.verify_cell_kzg_proof_batch(coms, idx, cells, prfs, s) is True
    texts(kzg, lambda: kzg.verify_cell_kzg_proof_batch(coms, idx, cells, PROBE["(0, 2)"] + prfs[48:], s), "Proof is not valid")
    texts(kzg, lambda: kzg.verify_cell_kzg_proof_batch(PROBE["order 11"] + coms[48:], idx, cells, prfs, s),
          "Commitment is not valid")
    assert kzg.verify_cell_kzg_proof_batch(coms, idx, cells, prfs, s) is True
