#!/usr/bin/env python3
"""Zero polynomials and sample recovery (kzgamd_poly_zero_poly, kzgamd_poly_recover) at the reference's bench shapes —
bench_zero_poly and bench_recover run at scale 15 with half of the points missing (kzg-bench/src/benches/zero_poly.rs,
recover.rs) — beside the time of the same batched transforms alone: the lengths and counts the call enqueues, through
kzgamd_ntt_fr_device on device buffers, in the same process, as tools/time_poly.py does for the polynomial rows.

  zero_poly_32768_form1, _form2   domain 2^15, 2^14 random missing indices, direct form and product tree
  recover_32768_x1, _x16          kzgamd_poly_recover, 2^15 samples with half missing, 1 and 16 vectors in a call
  recover_8192_x1, _x64           the same at 2^13, 1 and 64 vectors
  ..._loop                        beside each batch: the same vectors one call each ("transforms" is one call's list,
                                  "calls" says how many times the floor runs it)
  sweep_zero_<n>_<count>_form<f>  domain n = 2^10 and 2^15, count roots, both forms forced: ZP_DIRECT_MAX (zero_info) is
                                  the largest count at which the direct form is ahead (0: at none)

Recovery is defined for any sample values, so the samples are random field elements.  One process, legs alternating,
after warm-up; clock: the host's perf_counter around synchronous calls (every entry point returns when its output is in
host memory; the floor ends in a device synchronise).  One JSON line per row (median and spread = max - min of `reps`
runs, ms), appended to the output file.
python tools/time_zero_poly.py [reps >= 20] [output.jsonl]"""
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
from conftest import load_package


def random_frs(rnd, count):
    """count field elements (any value below 2^254 is one), as the library's buffers hold them"""
    raw = bytearray(rnd.randbytes(32 * count))
    raw[31::32] = bytes(b & 0x3F for b in raw[31::32])
    arr = (C.c_uint64 * (4 * max(1, count)))()
    C.memmove(arr, bytes(raw), len(raw))
    return arr


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "spread_ms": round(max(ts) - min(ts), 3), "runs": len(ts)}


def zero_transforms(kzg, n, count, nprob, direct):
    """(length, count, inverse) of the transforms a zero polynomial of `count` roots per problem enqueues, with its evaluation"""
    if direct:
        return [(n, nprob, 1)]
    out = []
    for npoly, _, tlen in kzg.PolySettings.zero_plan(count):
        out += [(tlen, 2 * (npoly // 2) * nprob, 0), (tlen, (npoly // 2) * nprob, 1)]
    return out + [(n, nprob, 0)]


def recover_transforms(kzg, n, count, nprob, direct_max):
    return zero_transforms(kzg, n, count, nprob, count <= direct_max) + [(n, nprob, 1), (n, 2 * nprob, 0), (n, nprob, 1), (n, nprob, 0)]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "zero_poly_time.jsonl")
    kzg = load_package()
    if kzg.device_count() < 1:
        raise SystemExit("time_zero_poly.py: no GPU visible; nothing is measured without one")
    import torch

    rnd = random.Random(26)
    fs = kzg.FFTSettings(15)
    ps = kzg.PolySettings(fs)
    leaf, direct_max = ps.zero_info()
    cap = 2 * 16 * (1 << 15) * 32   # the largest floor transforms 2 x 16 lists of 2^15 elements (= 2 x 64 of 2^13)
    d_in = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")

    def floor_of(transforms, calls):
        def run():
            for _ in range(calls):
                for n, count, inv in transforms:
                    fs.fft_fr_device(d_out.data_ptr(), d_in.data_ptr(), n, count, bool(inv))
                torch.cuda.synchronize()
        return run

    legs, keep = [], []
    L = kzg.lib()
    # outputs allocated once: a fresh ctypes array of 16 MB per call would be timed with it
    out_buf = (C.c_uint8 * (16 * (1 << 15) * 32))()
    ze_buf, zp_buf = (C.c_uint8 * ((1 << 15) * 32))(), (C.c_uint8 * ((1 << 15) * 32))()

    def zero_call(n, lst, form):
        marr = (C.c_uint64 * len(lst))(*lst)
        oarr = (C.c_size_t * 2)(0, len(lst))

        def run():
            rc = L.kzgamd_poly_zero_poly(ps.handle, ze_buf, zp_buf, n, marr, oarr, 1, form)
            assert rc == 0, rc
        return run

    def recover_call(addr, mask, n, nprob):
        marr = (C.c_uint8 * len(mask)).from_buffer_copy(mask)

        def run():
            rc = L.kzgamd_poly_recover(ps.handle, out_buf, addr, marr, n, nprob, 0)
            assert rc == 0, rc
        return run

    def leg(name, shape, call, transforms, calls=1):
        legs.append((name, shape, call, floor_of(transforms, calls), transforms))

    N15 = 1 << 15
    missing15 = rnd.sample(range(N15), N15 // 2)
    for form in (1, 2):
        leg("zero_poly_32768_form%d" % form, {"domain": N15, "missing": N15 // 2, "nprob": 1, "form": form},
            zero_call(N15, missing15, form), zero_transforms(kzg, N15, N15 // 2, 1, form == 1))
    for n, batch in ((N15, 16), (1 << 13, 64)):
        samples = random_frs(rnd, n * batch)
        present = bytearray()
        for _ in range(batch):
            gone = set(rnd.sample(range(n), n // 2))
            present += bytes(0 if i in gone else 1 for i in range(n))
        present = bytes(present)
        base = C.addressof(samples)
        keep.append(samples)

        singles = [recover_call(base + 32 * n * k, present[n * k: n * (k + 1)], n, 1) for k in range(batch)]

        def loop(singles=singles):
            for one in singles:
                one()

        leg("recover_%d_x1" % n, {"n": n, "missing": n // 2, "nprob": 1}, singles[0],
            recover_transforms(kzg, n, n // 2, 1, direct_max))
        leg("recover_%d_x%d" % (n, batch), {"n": n, "missing": n // 2, "nprob": batch},
            recover_call(base, present, n, batch), recover_transforms(kzg, n, n // 2, batch, direct_max))
        leg("recover_%d_x%d_loop" % (n, batch), {"n": n, "missing": n // 2, "nprob": batch, "calls": batch}, loop,
            recover_transforms(kzg, n, n // 2, 1, direct_max), calls=batch)
    for n in (1 << 10, N15):
        for count in (32, 64, 128, 256, 512):
            lst = rnd.sample(range(n), count)
            for form in (1, 2):
                leg("sweep_zero_%d_%d_form%d" % (n, count, form), {"domain": n, "missing": count, "nprob": 1, "form": form},
                    zero_call(n, lst, form), zero_transforms(kzg, n, count, 1, form == 1))

    for _, _, new, ref, _ in legs:  # warm-up: code objects, workspaces
        new()
        ref()
        new()
        ref()
    runs = {name: ([], []) for name, _, _, _, _ in legs}
    for _ in range(reps):
        for name, _, new, ref, _ in legs:
            t0 = time.perf_counter()
            new()
            t1 = time.perf_counter()
            ref()
            t2 = time.perf_counter()
            runs[name][0].append((t1 - t0) * 1e3)
            runs[name][1].append((t2 - t1) * 1e3)
    date = datetime.date.today().isoformat()
    with open(out_path, "a") as f:
        for name, shape, _, _, transforms in legs:
            new, ref = stats(runs[name][0]), stats(runs[name][1])
            row = {"date": date, "row": name, **shape, "leaf_roots": leaf, "direct_max": direct_max,
                   "clock": "host perf_counter around synchronous calls", "transforms": [list(t) for t in transforms],
                   "new": new, "transforms_alone": ref, "difference_ms": round(new["median_ms"] - ref["median_ms"], 3)}
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
    ps.close()
    fs.close()


if __name__ == "__main__":
    main()
