#!/usr/bin/env python3
"""kzgamd_g2_lincomb and kzgamd_verify_trusted_setup (setupcheck.hip) beside the host loop they replace, timed in one run.

kzgamd_g2_lincomb at 65, 2^12, 2^15 and 2^20 points (multiples of the generator by kzgamd_g2_mul_batch, Z != 1, random
scalars); kzgamd_verify_trusted_setup at (num_g1, num_g2) = (4096, 65), (2^15, 2^15) and (2^20, 65), with and without
the Lagrange form, on setups from kzgamd_generate_trusted_setup, with an explicit seed and with seed == NULL (which adds
the compression and the hash of every point).  Host clock around the synchronous calls, copies included, after one
warm-up call.  The host side is the loop kzgamd_p2_mult + kzgamd_p2_add over at most 256 points, extrapolated linearly
beyond that and marked as such; for a verification it is the two G2 combinations alone (2 (num_g2 - 1) terms), the part
of the check a host could not afford.
One JSON line per measurement: median, min and max of `reps` runs in ms.
python tools/time_setup_verify.py [reps] [output.jsonl]"""
import datetime
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_ffi as O
from conftest import load_package

R = O.R
HOST_MAX = 256
LINCOMB_COUNTS = (65, 1 << 12, 1 << 15, 1 << 20)
VERIFY_SIZES = ((4096, 65), (1 << 15, 1 << 15), (1 << 20, 65))


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


def host_row(fn, nhost, count, reps):
    ts = timed(fn, reps)
    per = statistics.median(ts) / nhost
    return {"loop": stats(ts), "points": nhost, "ms_per_point": round(per, 4), "ms_for_count": round(per * count, 3),
            "extrapolated": count > nhost}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "setup_verify_time.jsonl")
    kzg = load_package()
    if kzg.device_count() < 1:
        raise SystemExit("time_setup_verify.py: no GPU visible; nothing is measured without one")
    rnd = random.Random(40)
    date = datetime.date.today().isoformat()
    seed = hashlib.sha256(b"time_setup_verify").digest()
    with open(out_path, "a") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")

        def host_lincomb(pts, sc, nhost):
            acc = kzg.BlstP2()
            for i in range(nhost):
                acc = kzg.p2_add(acc, kzg.p2_mult(pts[i], sc[i]))
            return acc

        for count in LINCOMB_COUNTS:
            def scalars():
                raw = b"".join(((rnd.randrange(1, R) << 256) % R).to_bytes(32, "little") for _ in range(count))
                return (kzg.BlstFr * count).from_buffer_copy(raw)

            pts, sc = kzg.g2_mul_batch(scalars(), count), scalars()
            nhost = min(count, HOST_MAX)
            got = kzg.g2_lincomb(pts, sc, nhost)
            assert kzg.p2_compress(got) == kzg.p2_compress(host_lincomb(pts, sc, nhost)), "the host loop sums to another point"
            emit({"date": date, "what": "g2_lincomb", "count": count, "slice_points": kzg.g2_lincomb_info(),
                  "g2_lincomb": stats(timed(lambda: kzg.g2_lincomb(pts, sc, count), reps)),
                  "host_p2_mult_add": host_row(lambda: host_lincomb(pts, sc, nhost), nhost, count, reps)})

        for n1, n2 in VERIFY_SIZES:
            fs = kzg.FFTSettings(n1.bit_length() - 1)
            mono, lag, g2 = kzg.generate_trusted_setup(n1, hashlib.sha256(b"a secret").digest(), num_g2=n2, fft_settings=fs)
            assert kzg.verify_trusted_setup(mono, lag, g2, n1, n2, fft_settings=fs, seed=seed) == (0, 0)
            terms = 2 * (n2 - 1)
            nhost = min(terms, HOST_MAX)
            raw = b"".join(((rnd.randrange(1, R) << 256) % R).to_bytes(32, "little") for _ in range(nhost))
            sc = (kzg.BlstFr * nhost).from_buffer_copy(raw)
            emit({"date": date, "what": "verify_trusted_setup", "num_g1": n1, "num_g2": n2,
                  "with_lagrange": stats(timed(lambda: kzg.verify_trusted_setup(mono, lag, g2, n1, n2, fft_settings=fs, seed=seed), reps)),
                  "without_lagrange": stats(timed(lambda: kzg.verify_trusted_setup(mono, None, g2, n1, n2, seed=seed), reps)),
                  "with_lagrange_seed_null": stats(timed(lambda: kzg.verify_trusted_setup(mono, lag, g2, n1, n2, fft_settings=fs), reps)),
                  "host_g2_combinations": host_row(lambda: host_lincomb([g2[i % n2] for i in range(nhost)], sc, nhost), nhost, terms, reps)})
            fs.close()


if __name__ == "__main__":
    main()
