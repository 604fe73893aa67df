"""kzgamd_recover_cells_and_kzg_proofs_batch (recover_cells_and_kzg_proofs_batch, kzg/src/das.rs:209-241): n recoveries
in one call against the reference's vectors, against n single calls of recover_cells_and_kzg_proofs on the same settings
object, and against the cells and proofs the blobs had — under both proof forms (FK20 and the direct form, tuning key
fk20) on both sides of the batch size from which FK20 is the default.  Settings objects with 8 GB tables, as in
tests/test_switch_forms_gpu.py, so that the module fits next to nothing else."""
import ctypes as C
import gzip
import hashlib
import json
import os
import random

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
CELL = 2048
BLOB = 131072
SETUP = os.path.join(GOLDEN, "trusted_setup.txt")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
NULL = (2 ** 256 - 1) % R  # Fr::null() (blst/src/types/fr.rs:36-38)
COUNTS = (64, 65, 100, 127, 128)


@pytest.fixture(scope="module")
def forms(kzg):
    """default form / FK20 forced / direct cell proofs forced, each with 8 GB per table"""
    made = {}
    try:
        for name, tuning in (("default", None), ("fk20", {"fk20": 1}), ("direct", {"fk20": 0})):
            made[name] = kzg.KZGSettings.from_file(SETUP, kzg.make_config(table_budget_gb=8, tuning=tuning))
        yield made
    finally:
        for s in made.values():
            s.close()


def random_blobs(rnd, n):
    b = bytearray(rnd.randbytes(n * BLOB))
    for i in range(0, n * BLOB, 32):
        b[i] = 0
    return b


@pytest.fixture(scope="module")
def source(kzg, forms):
    """64 seeded blobs (blob 1 the zero polynomial: every proof is the point at infinity), their cells and proofs"""
    n = 64
    blobs = random_blobs(random.Random(7594), n)
    blobs[BLOB:2 * BLOB] = bytes(BLOB)
    blobs = bytes(blobs)
    cells, proofs = kzg.compute_cells_and_kzg_proofs_batch(blobs, n, forms["default"])
    assert proofs[6144:6144 + 48] == b"\xc0" + bytes(47)
    return [cells[b * 262144:(b + 1) * 262144] for b in range(n)], [proofs[b * 6144:(b + 1) * 6144] for b in range(n)]


def pick(cells, idx):
    return b"".join(cells[CELL * i:CELL * (i + 1)] for i in idx)


def singles(kzg, idx_list, cell_list, s):
    out = [kzg.recover_cells_and_kzg_proofs(ix, c, s) for ix, c in zip(idx_list, cell_list)]
    return [o[0] for o in out], [o[1] for o in out]


@pytest.mark.parametrize("form", ["default", "fk20", "direct"])
def test_reference_vectors_in_one_batch(kzg, forms, form):
    """The reference's four good recover_cells_and_kzg_proofs cases as one batch, then reversed and each twice (n = 8)."""
    with open(os.path.join(GOLDEN, "kzg_mainnet_7594.json")) as f:
        v = json.load(f)
    with gzip.open(os.path.join(GOLDEN, v["cells_file"]), "rb") as f:
        raw = f.read()
    pool = [raw[i:i + CELL] for i in range(0, len(raw), CELL)]
    cases = [c for c in v["recover_cells_and_kzg_proofs"]
             if c["output"] is not None and all(isinstance(r, int) for r in c["cells"]) and len(c["cells"]) == len(c["cell_indices"])]
    assert len(cases) == 4
    for order in (cases, [c for c in reversed(cases) for _ in range(2)]):
        got_c, got_p = kzg.recover_cells_and_kzg_proofs_batch([c["cell_indices"] for c in order],
                                                              [b"".join(pool[r] for r in c["cells"]) for c in order], forms[form])
        assert len(got_c) == len(order) == len(got_p)
        for c, gc, gp in zip(order, got_c, got_p):
            assert hashlib.sha256(gc).hexdigest() == c["output"]["cells_sha256"], c["name"]
            assert hashlib.sha256(gp).hexdigest() == c["output"]["proofs_sha256"], c["name"]


@pytest.mark.parametrize("form", ["default", "fk20", "direct"])
@pytest.mark.parametrize("shared", [True, False], ids=["same-columns", "own-columns"])
def test_equals_single_calls_and_the_original(kzg, forms, source, form, shared):
    """n in {1, 2, 3, 17, 64}, 64 ... 128 cells per blob: byte for byte what n single calls give on the same object, and
    the cells and proofs the blobs had (the zero blob included)."""
    s = forms[form]
    cells, proofs = source
    rnd = random.Random("%s/%s" % (form, shared))
    for n in (1, 2, 3, 17, 64):
        if shared:
            one = sorted(rnd.sample(range(128), rnd.choice(COUNTS)))
            idx = [one] * n
        else:
            idx = [sorted(rnd.sample(range(128), rnd.choice(COUNTS))) for _ in range(n)]
        given = [pick(cells[b], idx[b]) for b in range(n)]
        got_c, got_p = kzg.recover_cells_and_kzg_proofs_batch(idx, given, s)
        assert got_c == cells[:n], (n, [b for b in range(n) if got_c[b] != cells[b]])
        assert got_p == proofs[:n], (n, [b for b in range(n) if got_p[b] != proofs[b]])
        one_c, one_p = singles(kzg, idx, given, s)
        assert got_c == one_c and got_p == one_p, n


def test_without_proofs(kzg, forms, source):
    cells, _ = source
    rnd = random.Random(11)
    idx = [sorted(rnd.sample(range(128), k)) for k in (64, 128, 90, 127)]
    given = [pick(cells[b], idx[b]) for b in range(4)]
    for s in forms.values():
        with_p, _ = kzg.recover_cells_and_kzg_proofs_batch(idx, given, s)
        got, none = kzg.recover_cells_and_kzg_proofs_batch(idx, given, s, want_proofs=False)
        assert none is None and got == with_p == cells[:4]


@pytest.mark.parametrize("form", ["default", "fk20", "direct"])
def test_null_sentinel_valued_cell_element(kzg, forms, form):
    """As tests/test_cells7594_gpu.py::test_null_sentinel_valued_cell_element, inside one batch of 3: the blob with a
    Fr::null()-valued element given with all 128 cells (kept), the same blob with 64 cells (dropped), an ordinary blob."""
    s = forms[form]
    rnd = random.Random(77)
    blob = random_blobs(rnd, 1)
    blob[32 * 70:32 * 71] = NULL.to_bytes(32, "big")  # element 70 = cell 1, position 6
    other = bytes(random_blobs(rnd, 1))
    cells, proofs = kzg.compute_cells_and_kzg_proofs(bytes(blob), s)
    ocells, oproofs = kzg.compute_cells_and_kzg_proofs(other, s)
    idx = [list(range(128)), list(range(64)), sorted(rnd.sample(range(128), 100))]
    given = [cells, cells[:64 * CELL], pick(ocells, idx[2])]
    got_c, got_p = kzg.recover_cells_and_kzg_proofs_batch(idx, given, s)
    one_c, one_p = singles(kzg, idx, given, s)
    assert got_c == one_c and got_p == one_p
    assert got_c[0] == cells and got_p[0] == proofs
    assert got_c[1] != cells  # the reference's quirk: the dropped element changes the outcome
    assert got_c[2] == ocells and got_p[2] == oproofs


def test_bad_blob_fails_the_batch_and_the_object_recovers(kzg, source):
    """One bad blob in a batch of 4 (63 cells / unordered / repeated indices / index 128 / an element >= r): C_KZG_BADARGS.
    The same object then recovers good batches and single blobs correctly — before and after a larger batch has grown
    its workspace.  An object of its own, so that its workspace starts at its smallest."""
    cells, proofs = source
    s = kzg.KZGSettings.from_file(SETUP, kzg.make_config(table_budget_gb=8))
    try:
        rnd = random.Random(5)
        good_idx = [sorted(rnd.sample(range(128), k)) for k in (64, 100, 128, 77)]

        def good(b):
            return good_idx[b], pick(cells[b], good_idx[b])

        def bad_variants():
            ix = sorted(rnd.sample(range(128), 70))
            yield ix[:63], pick(cells[2], ix[:63])
            sw = ix[:]
            sw[10], sw[11] = sw[11], sw[10]
            yield sw, pick(cells[2], sw)
            dup = ix[:]
            dup[11] = dup[10]
            yield dup, pick(cells[2], dup)
            hi = sorted(rnd.sample(range(127), 69)) + [128]
            yield hi, pick(cells[2], hi[:-1]) + cells[2][:CELL]
            c = bytearray(pick(cells[2], ix))
            c[CELL * 5 + 32 * 9:CELL * 5 + 32 * 10] = b"\xff" * 32
            yield ix, bytes(c)
            c = bytearray(pick(cells[2], ix))
            c[CELL * 70 - 32:CELL * 70] = R.to_bytes(32, "big")  # r itself, as the last element of the last cell
            yield ix, bytes(c)

        def check_round():
            for bad_ix, bad_cells in bad_variants():
                idx = [good(b)[0] for b in range(4)]
                given = [good(b)[1] for b in range(4)]
                idx[2], given[2] = bad_ix, bad_cells
                with pytest.raises(kzg.KzgAmdError, match="C_KZG_RET 1$"):
                    kzg.recover_cells_and_kzg_proofs_batch(idx, given, s)
                got_c, got_p = kzg.recover_cells_and_kzg_proofs_batch([good(b)[0] for b in range(4)],
                                                                      [good(b)[1] for b in range(4)], s)
                assert got_c == cells[:4] and got_p == proofs[:4]
            assert kzg.recover_cells_and_kzg_proofs(*good(3), s) == (cells[3], proofs[3])

        check_round()
        n = 40
        idx = [sorted(rnd.sample(range(128), rnd.choice(COUNTS))) for _ in range(n)]
        got_c, got_p = kzg.recover_cells_and_kzg_proofs_batch(idx, [pick(cells[b], idx[b]) for b in range(n)], s)
        assert got_c == cells[:n] and got_p == proofs[:n]
        check_round()
    finally:
        s.close()


def test_empty_batch_and_null_output(kzg, forms, source):
    """n = 0 is C_KZG_OK; a NULL recovered_cells is C_KZG_BADARGS (through ctypes, below the Python wrapper)."""
    s = forms["default"]
    assert kzg.recover_cells_and_kzg_proofs_batch([], [], s) == ([], [])
    L = kzg.lib()
    out = C.create_string_buffer(128 * CELL)
    assert L.kzgamd_recover_cells_and_kzg_proofs_batch(out, None, None, None, None, 0, C.byref(s.c)) == kzg.C_KZG_OK
    cells, _ = source
    idx = list(range(64, 128))
    ix = (C.c_uint64 * 64)(*idx)
    num = (C.c_uint64 * 1)(64)
    given = pick(cells[0], idx)
    assert L.kzgamd_recover_cells_and_kzg_proofs_batch(None, None, ix, given, num, 1, C.byref(s.c)) == kzg.C_KZG_BADARGS
    assert L.kzgamd_recover_cells_and_kzg_proofs_batch(out, None, ix, given, num, 1, C.byref(s.c)) == kzg.C_KZG_OK
    assert out.raw == cells[0]
