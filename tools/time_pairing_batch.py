#!/usr/bin/env python3
"""Batched pairing checks on the GPU (kzgamd_pairings_verify_batch, one wave per check) beside a loop of the host's
kzgamd_pairings_verify on the same inputs, for count = 1, 4, 16, 64, 128, 1024, 4096.

One process, the two forms alternating, after warm-up (code objects, workspaces, the line tables of both G2 points on
the host and on the device); host clock around synchronous calls.  The items are e([k]G, [t]G2) against e([k t]G, G2)
with every third one off by one, Z != 1 on half of them; the verdicts of the two forms are compared once before the
timing.  The host loop is timed up to `host_max` checks (default 1024) and reported per check beyond that, marked as
such.  Then (kzg_rows) kzgamd_kzg_check with tuning key pairing_gpu_min = 1 against = 0, and a failing
kzgamd_kzg_check_batch with ok_each, on the README's shapes and at the counts around the threshold.  One JSON line per count (median, min, max of `reps` runs, ms), appended to the output file.
python tools/time_pairing_batch.py [reps] [output.jsonl] [host_max]"""
import datetime
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import g1_encodings as E
from conftest import load_package

COUNTS = (1, 4, 16, 64, 128, 1024, 4096)
T_SCALAR = 0x1F2E3D4C5B6A79880123456789ABCDEF


def p1_bytes(pt, z):
    vals = (pt[0] * z * z % E.P, pt[1] * z * z * z % E.P, z % E.P)
    return b"".join((v * (1 << 384) % E.P).to_bytes(48, "little") for v in vals)


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "runs": len(ts)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "pairing_batch_time.jsonl")
    host_max = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    kzg = load_package()
    if kzg.device_count() < 1:
        raise SystemExit("time_pairing_batch.py: no GPU visible; nothing is measured without one")
    rnd = random.Random(33)
    g2 = kzg.p2_generator()
    t_fr = kzg.BlstFr.from_buffer_copy(((T_SCALAR << 256) % E.R).to_bytes(32, "little"))
    qt = kzg.p2_mult(g2, t_fr)
    pool = []
    for i in range(24):
        k = rnd.randrange(1, E.R)
        z = 1 if i % 2 else rnd.randrange(2, 1 << 20)
        pool.append((p1_bytes(E.mul(k, E.G), z), p1_bytes(E.mul((k * T_SCALAR + (i % 3 == 0)) % E.R, E.G), z)))
    date = datetime.date.today().isoformat()
    with open(out_path, "a") as f:
        for count in COUNTS:
            items = [pool[rnd.randrange(len(pool))] for _ in range(count)]
            a1 = (kzg.BlstP1 * count).from_buffer_copy(b"".join(a for a, _ in items))
            b1 = (kzg.BlstP1 * count).from_buffer_copy(b"".join(b for _, b in items))
            nhost = min(count, host_max)

            def gpu():
                return kzg.pairings_verify_batch(a1, qt, b1, g2)

            def host():
                return [kzg.pairings_verify(a1[i], qt, b1[i], g2) for i in range(nhost)]

            assert gpu()[:nhost] == host(), "the two forms disagree"
            gpu()
            tg, th = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                gpu()
                t1 = time.perf_counter()
                host()
                t2 = time.perf_counter()
                tg.append((t1 - t0) * 1e3)
                th.append((t2 - t1) * 1e3)
            row = {"date": date, "row": "pairings_verify_batch", "count": count, "slice_checks": kzg.pairing_info(),
                   "gpu_batch": stats(tg), "host_loop": stats(th), "host_loop_checks": nhost,
                   "host_ms_per_check": round(statistics.median(th) / nhost, 4),
                   "gpu_ms_per_check": round(statistics.median(tg) / count, 4)}
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
    kzg_rows(kzg, reps, out_path, date)


def kzg_rows(kzg, reps, out_path, date):
    """kzgamd_kzg_check with pairing_gpu_min = 1 against = 0 (two handles over one setup of 1024 points) on 16 tuples of
    n = 64 and 64 tuples of n = 16, at further counts for the threshold, and a failing kzgamd_kzg_check_batch with ok_each"""
    import oracle_ffi as O
    from time_kzg import fr_bulk, setup_points

    R = O.R
    length = 1024
    rnd = random.Random(44)
    jac, _ = setup_points(length)
    g2gen = kzg.p2_generator()
    g2 = (kzg.BlstP2 * 65)()
    for i in range(65):
        g2[i] = kzg.p2_mult(g2gen, fr_bulk([pow(0x1234567, i, R)])[0])
    fs = kzg.FFTSettings(10)
    handles = {m: kzg.PolyKZGSettings(fs, jac, length, g2, 65, kzg.make_config(no_tables=True, tuning="pairing_gpu_min=%d" % m))
               for m in (1, 0)}
    fp = fr_bulk([rnd.randrange(R) for _ in range(length)])
    com1 = bytes(handles[0].commit(fp, length))[:144]
    shapes = [(64, 16), (16, 64)] + [(16, c) for c in (1, 2, 4, 6, 8, 12, 16, 32)] + [(1, c) for c in (4, 8, 16, 64, 256)]
    with open(out_path, "a") as f:
        for n, count in shapes:
            xs = fr_bulk([rnd.randrange(1, R) for _ in range(count)])
            proofs, ys = handles[0].open(fp, length, 1, xs, count, n)
            prf, yraw, com = bytes(proofs)[:144 * count], bytes(ys)[:32 * n * count], com1 * count
            bad = bytearray(yraw)
            bad[5] ^= 1  # tuple 0 fails: the batch fails and ok_each is asked for
            bad = bytes(bad)
            legs = [("check_gpu_min_1", lambda: handles[1].check(com, prf, xs, yraw, n, count)),
                    ("check_gpu_min_0", lambda: handles[0].check(com, prf, xs, yraw, n, count)),
                    ("failing_check_batch_ok_each_gpu_min_1", lambda: handles[1].check_batch(com, prf, xs, bad, n, count, each=True)),
                    ("failing_check_batch_ok_each_gpu_min_0", lambda: handles[0].check_batch(com, prf, xs, bad, n, count, each=True))]
            # the setup points are [i + 1]G as in tools/time_kzg.py, so the verdicts mean nothing here (every tuple fails);
            # the two forms must still agree, and warm up
            assert legs[0][1]() == legs[1][1]() and legs[2][1]() == legs[3][1](), "the two forms disagree"
            assert legs[2][1]()[0] is False
            ts = {name: [] for name, _ in legs}
            for _ in range(reps):
                for name, fn in legs:
                    t0 = time.perf_counter()
                    fn()
                    ts[name].append((time.perf_counter() - t0) * 1e3)
            row = {"date": date, "row": "kzg_check", "n": n, "count": count, "setup_points": length}
            row.update({name: stats(v) for name, v in ts.items()})
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
    for h in handles.values():
        h.close()
    fs.close()


if __name__ == "__main__":
    main()
