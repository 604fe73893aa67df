#!/usr/bin/env python3
"""kzgamd_verify_cell_kzg_proof_batch_many against what it replaces, in one process on one settings object, on the same
host buffers.  Cells and proofs of 64 random blobs (kzgamd_compute_cells_and_kzg_proofs_batch):
  a  128 batches x 64 cells: the data-column sidecars of a block of 64 blobs (batch c = column c of every blob, the 64
     commitments shared) against a loop of 128 verify_cell_kzg_proof_batch calls
  b  8 batches x 64 cells against a loop of 8 calls
  c  1 batch x 8192 cells, the reference's bench shape (kzg-bench/src/benches/eip_7594.rs:171-266: 64 blobs x 128 cells)
     against ONE verify_cell_kzg_proof_batch call on the same 8192 cells
  d  shape a with one wrong proof and ok_each requested: the cost of the per-batch fallback
Host clock around synchronous calls after two warm-up calls; min / median / max of `reps` calls for the new call and
for its comparison, and the median of the new call's stage times (kzgamd_vcells_timing).  One JSON line per shape.
python tools/time_verify_cells_many.py [reps] [shapes, e.g. abcd]"""
import ctypes as C
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package

CELL = 2048
BLOB = 131072
NBLOBS = 64


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    shapes = sys.argv[2] if len(sys.argv) > 2 else "abcd"
    kzg = load_package()
    L = kzg.lib()
    s = kzg.KZGSettings.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    sp = C.byref(s.c)
    try:
        rnd = random.Random(7594)
        blobs = bytearray(rnd.randbytes(NBLOBS * BLOB))
        for i in range(0, NBLOBS * BLOB, 32):
            blobs[i] = 0
        blobs = bytes(blobs)
        cells, proofs = kzg.compute_cells_and_kzg_proofs_batch(blobs, NBLOBS, s)
        cms = [kzg.blob_to_kzg_commitment(blobs[b * BLOB:(b + 1) * BLOB], s) for b in range(NBLOBS)]

        def cell(b, c):
            return cells[(b * 128 + c) * CELL:(b * 128 + c + 1) * CELL]

        def proof(b, c):
            return proofs[(b * 128 + c) * 48:(b * 128 + c + 1) * 48]

        def sidecar(c, wrong=False):
            prf = [proof(b, c) for b in range(NBLOBS)]
            if wrong:
                prf[17] = proof(17, (c + 1) % 128)
            return b"".join(cms), [c] * NBLOBS, b"".join(cell(b, c) for b in range(NBLOBS)), b"".join(prf)

        def measure(fn):
            fn()
            fn()
            ts, stages = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
                stages.append(kzg.vcells_timing(s))
            ts.sort()
            return ts, stages

        def spread(ts):
            return {"min_ms": round(ts[0], 3), "median_ms": round(ts[len(ts) // 2], 3), "max_ms": round(ts[-1], 3)}

        def run(shape, batches, expect, loop_is_one_call=False):
            n = len(batches)
            counts = [len(b[1]) for b in batches]
            flat = [i for b in batches for i in b[1]]
            idx = (C.c_uint64 * len(flat))(*flat)
            num = (C.c_uint64 * n)(*counts)
            coms, cls, prfs = (b"".join(b[k] for b in batches) for k in (0, 2, 3))
            ok, each = C.c_bool(False), (C.c_bool * n)()
            per = [((C.c_uint64 * len(b[1]))(*b[1]), b) for b in batches]
            single_ok = C.c_bool(False)
            f = L.verify_cell_kzg_proof_batch
            f.restype = C.c_int
            verdicts = [None] * n

            def many():
                assert L.kzgamd_verify_cell_kzg_proof_batch_many(C.byref(ok), each, coms, idx, cls, prfs, num, n, None, sp) == 0

            def many_g1():
                out = (kzg.BlstP1 * 2)()
                assert L.kzgamd_verify_cell_kzg_proof_batch_many_g1(out, coms, idx, cls, prfs, num, n, None, sp) == 0

            def loop():
                for j, (ix, b) in enumerate(per):
                    assert f(C.byref(single_ok), b[0], ix, b[2], b[3], C.c_uint64(len(b[1])), sp) == 0
                    verdicts[j] = bool(single_ok.value)

            t_many, stages = measure(many)
            got = (bool(ok.value), [bool(each[j]) for j in range(n)])
            t_g1, _ = measure(many_g1)
            t_loop, _ = measure(loop)
            assert got == (all(expect), expect) and verdicts == expect, shape
            med = {k: round(sorted(st[k] for st in stages)[len(stages) // 2], 3) for k in kzg.VCELLS_STAGES}
            row = {"shape": shape, "batches": n, "cells": len(flat), "reps": reps, "many": spread(t_many), "many_g1": spread(t_g1),
                   "compared_with": "one verify_cell_kzg_proof_batch call" if loop_is_one_call else "a loop of %d verify_cell_kzg_proof_batch calls" % n,
                   "comparison": spread(t_loop), "gain_of_medians": round(t_loop[len(t_loop) // 2] / t_many[len(t_many) // 2], 2),
                   "faster_beyond_spread": t_many[-1] < t_loop[0], "stage_median_ms": med, "verdicts_equal": True}
            print(json.dumps(row), flush=True)

        if "a" in shapes:
            run("a: 128 sidecars x 64 cells", [sidecar(c) for c in range(128)], [True] * 128)
        if "b" in shapes:
            run("b: 8 sidecars x 64 cells", [sidecar(c) for c in range(8)], [True] * 8)
        if "c" in shapes:
            one = (b"".join(cms[b] for b in range(NBLOBS) for _ in range(128)), [c for _ in range(NBLOBS) for c in range(128)], cells, proofs)
            run("c: 1 batch x 8192 cells", [one], [True], loop_is_one_call=True)
        if "d" in shapes:
            run("d: shape a, one wrong proof, ok_each", [sidecar(c, wrong=(c == 37)) for c in range(128)], [c != 37 for c in range(128)])
    finally:
        s.close()


if __name__ == "__main__":
    main()
