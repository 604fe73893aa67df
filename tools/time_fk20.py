#!/usr/bin/env python3
"""Generic FK20 (kzgamd_fk20_da) against the same proofs through the entry points the library had before it, in one
process, alternating, after warm-up.  Host clock around synchronous calls (every entry point returns when its output is
in host memory).

  new       kzgamd_fk20_da, direct form (fk20_table=0) and table form (fk20_table=1) where the table fits
  baseline  ntt_fr per Toeplitz vector -> kzgamd_prepare_msm_matrix (once) + kzgamd_mult_pippenger_matrix (rows = k2,
            cols = chunk_len) -> kzgamd_fft_g1_batch inverse -> upper halves zeroed -> kzgamd_fft_g1_batch forward, host
            buffers between them.  The Toeplitz vectors are gathered BEFORE the clock starts (in favour of the baseline);
            the transposition of the transformed coefficients (numpy) is inside it.
  cells     at (8192, 64) also kzgamd_compute_cells_and_kzg_proofs_batch on blobs with the same polynomials (recorded,
            not compared: it also produces the cells and compresses its proofs)

Shapes: the reference's bench shapes (kzg-bench/src/benches/fk20.rs: single n2 = 2^14; multi n = 2^14, chunk_len 16), the
cell shape (8192, 64) with 1 / 16 / 64 polynomials, single n2 = 2^16 (direct form only).  The setup points are [i + 1]G
(valid G1 points; the time does not depend on their values); new and baseline outputs are compared as group elements.
One JSON line per (shape, leg): median and spread (max - min) of `reps` runs in ms.
python tools/time_fk20.py [reps] [shape,shape,...]"""
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_ffi as O
from conftest import load_package

R = O.R
SHAPES = {  # name: (scale, n2, chunk_len, npoly, table form too)
    "single_2p14": (14, 1 << 14, 1, 1, True),
    "multi_2p14_16": (15, 1 << 15, 16, 1, True),
    "cells_1": (13, 8192, 64, 1, True),
    "cells_16": (13, 8192, 64, 16, True),
    "cells_64": (13, 8192, 64, 64, True),
    "single_2p16": (16, 1 << 16, 1, 1, False),
}


def setup_points(n):
    L = O.lib()
    g = O.G1()
    L.og1_generator(C.byref(g))
    arr = (O.G1 * n)()
    cur = O.G1()
    C.memmove(C.byref(cur), C.byref(g), 144)
    for i in range(n):
        C.memmove(C.byref(arr[i]), C.byref(cur), 144)
        nxt = O.G1()
        L.og1_add_or_dbl(C.byref(nxt), C.byref(cur), C.byref(g))
        cur = nxt
    return arr


def fr_bulk(vals):
    raw = b"".join(((v << 256) % R).to_bytes(32, "little") for v in vals)
    arr = (O.Fr * len(vals))()
    C.memmove(arr, raw, len(raw))
    return arr


def toeplitz(p, i, l):
    n = len(p)
    k = n // l
    t = [0] * (2 * k)
    t[0] = p[n - 1 - i]
    for idx in range(k + 2, 2 * k):
        t[idx] = p[n - 1 - i - l * (2 * k - idx)]
    return t


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "spread_ms": round(max(ts) - min(ts), 3), "runs": len(ts)}


def main():
    import torch

    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    names = sys.argv[2].split(",") if len(sys.argv) > 2 else list(SHAPES)
    kzg = load_package()
    L, OL = kzg.lib(), O.lib()
    mono = setup_points(1 << 15)
    rnd = random.Random(20)
    fs_by_scale = {}
    for name in names:
        scale, n2, l, npoly, with_table = SHAPES[name]
        n, k = n2 // 2, n2 // 2 // l
        k2 = 2 * k
        fs = fs_by_scale.get(scale) or kzg.FFTSettings(scale)
        fs_by_scale[scale] = fs
        polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(npoly)]
        flat = fr_bulk([c for p in polys for c in p])
        free_gb = torch.cuda.mem_get_info(0)[0] / 1e9
        min_gb = n2 * 512 * 13 * 128 / 1e9
        fits = with_table and (free_gb - 12) / 1.05 > min_gb * 1.02 + 4
        row = {"shape": name, "n2": n2, "chunk_len": l, "npoly": npoly}
        legs = {}
        outs = {}
        # ---- new
        for form in ("direct", "table"):
            if form == "table" and not fits:
                continue
            cfg = kzg.make_config(tuning={"fk20_table": 0}) if form == "direct" else \
                kzg.make_config(table_budget_gb=min_gb * 1.02, tuning={"fk20_table": 1})
            fk = kzg.FK20Settings(fs, mono, n - l, n2, l, cfg)
            legs[form] = (fk, lambda fk=fk: outs.__setitem__("new", fk.data_availability(flat, npoly, optimized=True)))
        # ---- baseline (entry points of the parent): X by fft_g1, matrix handle, host round trips
        base = None
        if fits:
            x = (O.G1 * (l * k2))()
            for i in range(l):
                for m in range(k - 1):
                    C.memmove(C.byref(x[i * k2 + m]), C.byref(mono[n - l - 1 - i - l * m]), 144)
            X = fs.fft_g1(x, k2, nbatch=l)
            aff = (O.G1Affine * (k2 * l))()
            Xg = C.cast(X, C.POINTER(O.G1))
            for j in range(k2):
                for i in range(l):
                    OL.og1_to_affine(C.byref(aff[j * l + i]), C.byref(Xg[i * k2 + j]))
            mat = kzg.MatrixMsm(aff, k2, l, kzg.make_config(table_budget_gb=min_gb * 1.02))
            tvecs = [fr_bulk(toeplitz(p, i, l)) for p in polys for i in range(l)]

            def baseline():
                tr = np.empty((npoly, l, k2, 32), dtype=np.uint8)
                for q, tv in enumerate(tvecs):
                    tr[q // l, q % l] = np.frombuffer(fs.fft_fr(tv, k2), dtype=np.uint8).reshape(k2, 32)
                sc = np.ascontiguousarray(tr.transpose(0, 2, 1, 3))
                h_ext = mat.multiply_batch(sc.ctypes.data, npoly)
                h = fs.fft_g1(h_ext, k2, inverse=True, nbatch=npoly)
                hv = np.frombuffer(h, dtype=np.uint8).reshape(npoly, k2, 144)
                hv[:, k:, :] = 0
                outs["base"] = fs.fft_g1(h, k2, nbatch=npoly)

            base = baseline
        cells = None
        if (n2, l) == (8192, 64) and os.environ.get("KZGAMD_TIME_FK20_CELLS", "1") == "1":
            # blobs with these polynomials: evaluations in bit-reversed order, big-endian
            s = kzg.KZGSettings.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"), kzg.make_config(table_budget_gb=8))
            blobs = bytearray()
            unmont = pow(1 << 256, R - 2, R)
            for p in polys:
                ev = fs.fft_fr(fr_bulk(p), 4096)
                ints = [int.from_bytes(bytes(ev[i]), "little") * unmont % R for i in range(4096)]
                for i in range(4096):
                    blobs += ints[int(format(i, "012b")[::-1], 2)].to_bytes(32, "big")
            blobs = bytes(blobs)
            cells = (s, lambda: kzg.compute_cells_and_kzg_proofs_batch(blobs, npoly, s))
        # ---- alternate the legs
        runs = {key: [] for key in list(legs) + (["baseline"] if base else []) + (["cells_batch"] if cells else [])}
        for key, (_, fn) in legs.items():
            fn()
        if base:
            base()
        if cells:
            cells[1]()
        for _ in range(reps):
            for key, (_, fn) in legs.items():
                t0 = time.perf_counter()
                fn()
                runs[key].append((time.perf_counter() - t0) * 1e3)
            if base:
                t0 = time.perf_counter()
                base()
                runs["baseline"].append((time.perf_counter() - t0) * 1e3)
            if cells:
                t0 = time.perf_counter()
                cells[1]()
                runs["cells_batch"].append((time.perf_counter() - t0) * 1e3)
        for key, ts in runs.items():
            row[key] = stats(ts)
        if base:
            a = C.cast(outs["new"], C.POINTER(O.G1))
            b = C.cast(outs["base"], C.POINTER(O.G1))
            row["new_equals_baseline"] = all(
                bool(OL.og1_equal(C.byref(a[j]), C.byref(b[j]))) or (OL.og1_is_inf(C.byref(a[j])) and OL.og1_is_inf(C.byref(b[j])))
                for j in range(0, npoly * k2, max(1, npoly * k2 // 512)))
        print(json.dumps(row), flush=True)
        for fk, _ in legs.values():
            fk.close()
        if base:
            mat.close()
        if cells:
            cells[0].close()
    for fs in fs_by_scale.values():
        fs.close()


if __name__ == "__main__":
    main()
