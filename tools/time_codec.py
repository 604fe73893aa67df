#!/usr/bin/env python3
"""The batched codec calls (codec.hip) beside the per-point host work they replace, timed in the same run.

G1 at 1, 65, 4096, 2^15 and 2^20 points, G2 at 1, 65, 4096 and 2^15: kzgamd_g1_uncompress_batch with and without the
subgroup test, kzgamd_g1_compress_batch, kzgamd_g1_to_affine_batch, kzgamd_g2_uncompress_batch with and without the
test, kzgamd_g2_compress_batch.  Host clock around the synchronous calls, copies included, after one warm-up call.
The host side is a loop over at most 256 points, extrapolated linearly beyond that and marked as such (as
tools/time_pairing_batch.py does): the CPU oracle's og1_uncompress + og1_in_subgroup / og1_compress for G1, the
library's own kzgamd_p2_uncompress (+ kzgamd_p2_in_g2) / kzgamd_p2_compress for G2.  The points are multiples of the
generators by kzgamd_g1_mul_batch / kzgamd_g2_mul_batch (Z != 1), so compress has an inversion to do.
One JSON line per (group, count): median, min and max of `reps` runs in ms.
python tools/time_codec.py [reps] [output.jsonl]"""
import ctypes as C
import datetime
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
G1_COUNTS = (1, 65, 4096, 1 << 15, 1 << 20)
G2_COUNTS = (1, 65, 4096, 1 << 15)


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
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "codec_time.jsonl")
    kzg = load_package()
    if kzg.device_count() < 1:
        raise SystemExit("time_codec.py: no GPU visible; nothing is measured without one")
    rnd = random.Random(39)
    L = O.lib()
    date = datetime.date.today().isoformat()
    with open(out_path, "a") as f:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")

        for count in G1_COUNTS:
            raw = b"".join(((rnd.randrange(1, R) << 256) % R).to_bytes(32, "little") for _ in range(count))
            sc = (kzg.BlstFr * count).from_buffer_copy(raw)
            pts = kzg.g1_mul_batch(sc, count)
            data = kzg.g1_compress_batch(pts, count)
            nhost = min(count, HOST_MAX)
            g = O.G1()
            C.memmove(C.byref(g), bytes(pts[0]), 144)
            buf = C.create_string_buffer(48)
            L.og1_compress(buf, C.byref(g))
            assert buf.raw == data[:48], "the oracle compresses the first point to other bytes"
            decoded, status, rc = kzg.g1_uncompress_batch(data, True)
            assert rc == 0 and kzg.g1_compress_batch(decoded, count) == data

            def host_parse(check):
                a, j = O.G1Affine(), O.G1()
                for i in range(nhost):
                    L.og1_uncompress(C.byref(a), data[48 * i:48 * i + 48])
                    L.og1_from_affine(C.byref(j), C.byref(a))
                    if check:
                        L.og1_in_subgroup(C.byref(j))

            def host_compress():
                j, o = O.G1(), C.create_string_buffer(48)
                for i in range(nhost):
                    C.memmove(C.byref(j), C.byref(pts[i]), 144)
                    L.og1_compress(o, C.byref(j))

            emit({"date": date, "group": "G1", "count": count, "slice_points": kzg.codec_info(),
                  "uncompress_checked": stats(timed(lambda: kzg.g1_uncompress_batch(data, True), reps)),
                  "uncompress_unchecked": stats(timed(lambda: kzg.g1_uncompress_batch(data, False), reps)),
                  "compress": stats(timed(lambda: kzg.g1_compress_batch(pts, count), reps)),
                  "to_affine": stats(timed(lambda: kzg.g1_to_affine_batch(pts, count), reps)),
                  "host_uncompress_checked": host_row(lambda: host_parse(True), nhost, count, reps),
                  "host_uncompress_unchecked": host_row(lambda: host_parse(False), nhost, count, reps),
                  "host_compress": host_row(host_compress, nhost, count, reps)})
        for count in G2_COUNTS:
            raw = b"".join(((rnd.randrange(1, R) << 256) % R).to_bytes(32, "little") for _ in range(count))
            sc = (kzg.BlstFr * count).from_buffer_copy(raw)
            pts = kzg.g2_mul_batch(sc, count)
            data = kzg.g2_compress_batch(pts, count)
            nhost = min(count, HOST_MAX)
            assert kzg.p2_compress(pts[0]) == data[:96]
            decoded, status, rc = kzg.g2_uncompress_batch(data, True)
            assert rc == 0 and kzg.g2_compress_batch(decoded, count) == data

            def host_parse2(check):
                for i in range(nhost):
                    p = kzg.p2_uncompress(data[96 * i:96 * i + 96])
                    if check:
                        kzg.p2_in_g2(p)

            def host_compress2():
                for i in range(nhost):
                    kzg.p2_compress(pts[i])

            emit({"date": date, "group": "G2", "count": count, "slice_points": kzg.codec_info(),
                  "uncompress_checked": stats(timed(lambda: kzg.g2_uncompress_batch(data, True), reps)),
                  "uncompress_unchecked": stats(timed(lambda: kzg.g2_uncompress_batch(data, False), reps)),
                  "compress": stats(timed(lambda: kzg.g2_compress_batch(pts, count), reps)),
                  "host_uncompress_checked": host_row(lambda: host_parse2(True), nhost, count, reps),
                  "host_uncompress_unchecked": host_row(lambda: host_parse2(False), nhost, count, reps),
                  "host_compress": host_row(host_compress2, nhost, count, reps)})


if __name__ == "__main__":
    main()
