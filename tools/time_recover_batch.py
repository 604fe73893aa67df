#!/usr/bin/env python3
"""kzgamd_recover_cells_and_kzg_proofs_batch against a loop of n recover_cells_and_kzg_proofs calls, in one process on one
settings object: the reference's "whole matrix" shapes (kzg-bench/src/benches/eip_7594.rs:120-140: every blob of a block,
cells i with i % k == 0 missing, k = 2 / 4 / 8 -> 50 / 25 / 12.5 % missing).  Host clock around synchronous calls
(both entry points return when their outputs are in host memory), after warm-up; the outputs of the two are compared.
One JSON line per (n, % missing).  python tools/time_recover_batch.py [n,n,...] [reps]"""
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


def main():
    sizes = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [1, 4, 16, 64, 128]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    kzg = load_package()
    L = kzg.lib()
    s = kzg.KZGSettings.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    try:
        nmax = max(sizes)
        rnd = random.Random(7594)
        blobs = bytearray(rnd.randbytes(nmax * BLOB))
        for i in range(0, nmax * BLOB, 32):
            blobs[i] = 0
        cells, proofs = kzg.compute_cells_and_kzg_proofs_batch(bytes(blobs), nmax, s)
        for k in (2, 4, 8):
            idx = [i for i in range(128) if i % k != 0]
            ix = (C.c_uint64 * len(idx))(*idx)
            given = [b"".join(cells[b * 262144 + CELL * i:b * 262144 + CELL * (i + 1)] for i in idx) for b in range(nmax)]
            for n in sizes:
                flat_ix = (C.c_uint64 * (n * len(idx)))(*(idx * n))
                num = (C.c_uint64 * n)(*([len(idx)] * n))
                flat_cells = b"".join(given[:n])
                bc, bp = C.create_string_buffer(n * 128 * CELL), C.create_string_buffer(n * 128 * 48)
                sc, sp = C.create_string_buffer(n * 128 * CELL), C.create_string_buffer(n * 128 * 48)
                sc_addr, sp_addr = C.addressof(sc), C.addressof(sp)

                def batch():
                    assert L.kzgamd_recover_cells_and_kzg_proofs_batch(bc, bp, flat_ix, flat_cells, num, n, C.byref(s.c)) == 0

                def loop():
                    f = L.recover_cells_and_kzg_proofs
                    for b in range(n):
                        rc = f(C.c_void_p(sc_addr + b * 128 * CELL), C.c_void_p(sp_addr + b * 128 * 48), ix, given[b],
                               C.c_uint64(len(idx)), C.byref(s.c))
                        assert rc == 0

                def timed(fn):
                    fn()
                    fn()
                    ts = []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        fn()
                        ts.append(time.perf_counter() - t0)
                    ts.sort()
                    return ts[len(ts) // 2] * 1e3

                t_batch = timed(batch)
                t_loop = timed(loop)
                same = bc.raw == sc.raw and bp.raw == sp.raw
                orig = bc.raw == cells[:n * 128 * CELL] and bp.raw == proofs[:n * 128 * 48]
                print(json.dumps({"n": n, "missing_pct": 100.0 / k, "cells_given": len(idx), "batch_ms": round(t_batch, 3),
                                  "loop_ms": round(t_loop, 3), "batch_ms_per_blob": round(t_batch / n, 3),
                                  "loop_ms_per_blob": round(t_loop / n, 3), "gain": round(t_loop / t_batch, 2),
                                  "outputs_equal": same, "equal_to_original": orig}), flush=True)
                assert same and orig, (n, k)
    finally:
        s.close()


if __name__ == "__main__":
    main()
