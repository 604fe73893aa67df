#!/usr/bin/env python3
"""kzgamd_g2_msm (g2msm.hip: the prepared bucket MSM in G2) beside kzgamd_g2_lincomb (setupcheck.hip: a lane per point
walks its scalar) on the same inputs, timed in one run.

65, 2^12, 2^15 and 2^20 points at nbatch 1 and 2^15 points at nbatch 16 (the walk: 16 calls), the creation of the handle
at each count, and a sweep of g2msm_segment over 4, 8, 16, 32, 64 at 2^15 and 2^20 points.  Points are multiples of the
generator by kzgamd_g2_mul_batch (Z = 1 as that call leaves them), scalars random.  Host clock around the synchronous
calls, pageable buffers, copies included; median, min and max of `reps` runs in ms after one warm-up call.  Before
anything is timed the two calls must agree on every input.
One JSON line per measurement.
python tools/time_g2_msm.py [reps] [output.jsonl] [largest log2 count] [log2 counts of a sweep alone, e.g. 12,17,18]"""
import datetime
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package

COUNTS = (65, 1 << 12, 1 << 15, 1 << 20)
BATCH = (1 << 15, 16)
SEGMENTS = (4, 8, 16, 32, 64)
SWEEP_COUNTS = (1 << 15, 1 << 20)


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
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "g2_msm_time.jsonl")
    max_log = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    sweep_counts = [1 << int(k) for k in sys.argv[4].split(",")] if len(sys.argv) > 4 else SWEEP_COUNTS
    counts = COUNTS if len(sys.argv) <= 4 else ()  # a sweep at other counts is a run of its own
    kzg = load_package()
    if kzg.device_count() < 1:
        raise SystemExit("time_g2_msm.py: no GPU visible; nothing is measured without one")
    rnd = random.Random(44)
    date = datetime.date.today().isoformat()

    def scalars(count):
        """Montgomery blst_fr: any 32 bytes below 2^254 < r are the form of some scalar"""
        raw = bytearray(rnd.randbytes(32 * count))
        raw[31::32] = bytes(b & 0x3f for b in raw[31::32])
        return (kzg.BlstFr * count).from_buffer_copy(raw)

    with open(out_path, "a") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")

        def created(pts, count, config=None):
            made = []

            def once():
                if made:
                    made.pop().close()
                made.append(kzg.G2Msm(pts, count, config))

            ts = timed(once, reps)
            return made[0], ts

        def agree(h, pts, sc, count):
            got = h.g2_msm(sc, count, 1)
            assert kzg.p2_compress(got[0]) == kzg.p2_compress(kzg.g2_lincomb(pts, sc, count)), "the two calls sum to different points"

        inputs = {}
        for count in counts:
            if count > 1 << max_log:
                continue
            pts, sc = kzg.g2_mul_batch(scalars(count), count), scalars(count)
            inputs[count] = (pts, sc)
            h, create = created(pts, count)
            agree(h, pts, sc, count)
            info = h.info()
            emit({"date": date, "what": "g2_msm", "count": count, "nbatch": 1, "segment": info["segment"], "pass_entries": info["pass_entries"],
                  "table_bytes": info["table_bytes"], "create": stats(create),
                  "g2_msm": stats(timed(lambda: h.g2_msm(sc, count, 1), reps)),
                  "g2_lincomb": stats(timed(lambda: kzg.g2_lincomb(pts, sc, count), reps))})
            if count == BATCH[0]:
                nb = BATCH[1]
                scb = scalars(count * nb)
                rows = [(kzg.BlstFr * count).from_buffer_copy(bytes(scb)[32 * count * b:32 * count * (b + 1)]) for b in range(nb)]
                got = h.g2_msm(scb, count, nb)
                for b in (0, nb - 1):
                    assert kzg.p2_compress(got[b]) == kzg.p2_compress(kzg.g2_lincomb(pts, rows[b], count)), b
                emit({"date": date, "what": "g2_msm", "count": count, "nbatch": nb, "segment": info["segment"],
                      "g2_msm": stats(timed(lambda: h.g2_msm(scb, count, nb), reps)),
                      "g2_lincomb_calls": stats(timed(lambda: [kzg.g2_lincomb(pts, r, count) for r in rows], reps))})
            h.close()

        for count in sweep_counts:
            if count > 1 << max_log:
                continue
            if count not in inputs:
                inputs[count] = (kzg.g2_mul_batch(scalars(count), count), scalars(count))
            pts, sc = inputs[count]
            row = {"date": date, "what": "g2msm_segment sweep", "count": count, "nbatch": 1}
            for seg in SEGMENTS:
                h = kzg.G2Msm(pts, count, kzg.make_config(tuning="g2msm_segment=%d" % seg))
                agree(h, pts, sc, count)
                row["segment_%d" % seg] = stats(timed(lambda: h.g2_msm(sc, count, 1), reps))
                h.close()
            emit(row)


if __name__ == "__main__":
    main()
