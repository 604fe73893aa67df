#!/usr/bin/env python3
"""Trusted setups on the GPU (kzgamd_generate_trusted_setup) and the two batched multiplications under them
(kzgamd_g1_mul_batch, kzgamd_g2_mul_batch), beside the host loops they replace.

One process; per row a warm-up call (code objects, the generators' tables, the NTT handle's roots) and then `reps` timed
calls (default 10), host clock around the synchronous calls, median / min / max in ms.
  setup rows   num_g1 = 2^12, 2^14, 2^15, 2^20 with num_g2 = 65 and num_g2 = num_g1 (2^20: 65 only), with and without
               the Lagrange form;
  mul rows     the two _mul_batch calls alone at the same counts, on the scalars s^i of the setup;
  host rows    on the same scalars, in the same run: kzgamd_p2_mult per G2 point (the product's host code) and the CPU
               oracle's og1_mul per G1 point (labelled "port", as bench.py's cpu_baseline is).  `host_points` of each
               (default 256) are timed and the loop over the whole count is EXTRAPOLATED linearly from them; the record
               says so ("extrapolated_from").
Each record carries the ratio host G2 loop / GPU call.  One JSON line per row, appended to the output file.
python tools/bench_setup_gen.py [reps] [output.jsonl] [host_points] [log2 sizes, comma separated]"""
import ctypes as C
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_ffi as O
from conftest import load_package

R = O.R
SECRET = bytes([0xA4, 0x73, 0x31, 0x95, 0x28, 0xC8, 0xB6, 0xEA, 0x4D, 0x08, 0xCC, 0x53, 0x18] + [0] * 19)  # the reference's


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "runs": len(ts)}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "setup_gen_time.jsonl")
    host_points = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    logs = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [12, 14, 15, 20]
    kzg = load_package()
    if kzg.device_count() < 1:
        raise SystemExit("bench_setup_gen.py: no GPU visible; nothing is measured without one")
    L = kzg.lib()
    s = int.from_bytes(SECRET, "big") % R
    date = datetime.date.today().isoformat()
    info = kzg.group_mul_info()

    # ---- the host loops, per point, on the first host_points scalars s^i
    pw = []
    v = 1
    for _ in range(host_points):
        pw.append(v)
        v = v * s % R
    frs = (kzg.BlstFr * host_points).from_buffer_copy(b"".join(((x << 256) % R).to_bytes(32, "little") for x in pw))
    g2 = kzg.p2_generator()
    t0 = time.perf_counter()
    host_g2 = [kzg.p2_mult(g2, frs[i]) for i in range(host_points)]
    host_g2_ms = (time.perf_counter() - t0) * 1e3 / host_points
    OL = O.lib()
    gen, out = O.G1(), O.G1()
    OL.og1_generator(C.byref(gen))
    ofr = [O.fr_from_int(x) for x in pw]
    t0 = time.perf_counter()
    for f in ofr:
        OL.og1_mul(C.byref(out), C.byref(gen), C.byref(f))
    port_g1_ms = (time.perf_counter() - t0) * 1e3 / host_points
    # the GPU's answers on those scalars are the host's
    got = kzg.g2_mul_batch(frs, host_points)
    assert all(kzg.p2_compress(got[i]) == kzg.p2_compress(host_g2[i]) for i in range(host_points)), "G2: GPU and host disagree"

    with open(out_path, "a") as f:
        def emit(row):
            row.update({"date": date, "host_g2_ms_per_point": round(host_g2_ms, 4), "port_g1_ms_per_point": round(port_g1_ms, 4),
                        "extrapolated_from": host_points, "window_bits": [info["g1_window_bits"], info["g2_window_bits"]],
                        "slice_points": info["slice_points"]})
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")

        for lg in logs:
            n = 1 << lg
            fs = kzg.FFTSettings(lg)
            mono, lag = (kzg.BlstP1 * n)(), (kzg.BlstP1 * n)()
            for num_g2 in ((65,) if lg >= 20 else (65, n)):
                g2buf = (kzg.BlstP2 * num_g2)()
                for lagrange in (True, False):
                    def call():
                        rc = L.kzgamd_generate_trusted_setup(fs.handle, mono, lag if lagrange else None, g2buf, n, num_g2, SECRET, None)
                        assert rc == 0, rc

                    ts = timed(call, reps)
                    med = statistics.median(ts)
                    emit({"row": "generate_trusted_setup", "num_g1": n, "num_g2": num_g2, "lagrange": lagrange, "gpu": stats(ts),
                          "host_g2_loop_ms": round(host_g2_ms * num_g2, 1), "port_g1_loop_ms": round(port_g1_ms * n, 1),
                          "host_g2_loop_over_gpu": round(host_g2_ms * num_g2 / med, 2),
                          "host_both_loops_over_gpu": round((host_g2_ms * num_g2 + port_g1_ms * n) / med, 2)})
                del g2buf
            # the two multiplications alone, on the monomial scalars (computed once on the host for the upload)
            raw = bytearray(32 * n)
            v = 1
            for i in range(n):
                raw[32 * i:32 * i + 32] = ((v << 256) % R).to_bytes(32, "little")
                v = v * s % R
            sc = (kzg.BlstFr * n).from_buffer_copy(bytes(raw))
            g2out = (kzg.BlstP2 * n)()

            def call_g1():
                assert L.kzgamd_g1_mul_batch(mono, None, sc, n, None) == 0

            def call_g2():
                assert L.kzgamd_g2_mul_batch(g2out, None, sc, n, None) == 0

            t1, t2 = timed(call_g1, reps), timed(call_g2, reps)
            emit({"row": "g1_mul_batch", "n": n, "gpu": stats(t1), "port_g1_loop_ms": round(port_g1_ms * n, 1),
                  "port_loop_over_gpu": round(port_g1_ms * n / statistics.median(t1), 2)})
            emit({"row": "g2_mul_batch", "n": n, "gpu": stats(t2), "host_g2_loop_ms": round(host_g2_ms * n, 1),
                  "host_loop_over_gpu": round(host_g2_ms * n / statistics.median(t2), 2)})
            del sc, g2out, mono, lag
            fs.close()


if __name__ == "__main__":
    main()
