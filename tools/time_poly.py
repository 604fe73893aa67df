#!/usr/bin/env python3
"""Batched polynomial arithmetic (kzgamd_poly_*) at the reference's bench shape — bench_new_poly_div divides 2^15
coefficients by 2^14 (kzg-bench/src/benches/poly.rs) — beside the time of the same transforms alone: the lengths and
counts the call enqueues, through kzgamd_ntt_fr_device on device buffers, in the same process.  That is the floor a
call is compared with, as tools/time_kzg.py compares an open with its MSM; the difference is what the uploads, the
padding / pointwise / cut kernels, the recurrence of the inverse and the download cost.

  div_1, div_16      kzgamd_poly_div, 2^15 by 2^14, one polynomial and 16 in a call
  mul_16k            kzgamd_poly_mul, 2^14 x 2^14 -> 2^15 - 1 coefficients (form 0)
  inverse_16k1       kzgamd_poly_inverse of 2^14 coefficients to 2^14 + 1
  eval_1, eval_16    kzgamd_poly_eval, 2^15 coefficients at 1 and at 16 points (no transform: the floor is 0)

and the sweeps the thresholds of rust-kzg_amd/csrc/poly.hip are set from:

  sweep_mul_n        n x n -> 2n - 1 with form 1 (direct) and form 2 (transforms) forced: MUL_DIRECT_MAX is the largest n
                     at which the direct form is not slower
  sweep_inverse_L    inverse of 40 coefficients to L = 16, 32, 64 (recurrence alone: L - 1 dependent steps in one
                     launch) and 128, 256 (64 by the recurrence, then one and two Newton steps): INV_DIRECT_MAX = 64 is
                     right while 32 more steps of the recurrence cost less than a Newton step
  sweep_eval_len     eval at one point of 2^10 .. 2^15 coefficients: the depth of the chunk (CHUNK, shared with kzg.hip)
                     plus the scan

One process, legs alternating, after warm-up; host clock around synchronous calls (every entry point returns when its
output is in host memory; the floor ends in a device synchronise).  One JSON line per row (median and spread = max - min
of `reps` runs, ms), appended to the output file.
python tools/time_poly.py [reps] [output.jsonl]"""
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
import poly_model as P
from conftest import load_package

R = P.R


def fr_bulk(vals):
    raw = b"".join(((v << 256) % R).to_bytes(32, "little") for v in vals)
    arr = (C.c_uint64 * (4 * max(1, len(vals))))()
    C.memmove(arr, raw, len(raw))
    return arr


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "spread_ms": round(max(ts) - min(ts), 3), "runs": len(ts)}


def mul_transforms(la, lb, out_len, npoly, mul_max, form=0):
    """(length, count, inverse) of the transforms kzgamd_poly_mul enqueues"""
    ca, cb = min(la, out_len), min(lb, out_len)
    if ca + cb - 1 < 2 or form == 1 or (form == 0 and min(ca, cb) <= mul_max):
        return []
    n = P.next_pow_of_2(ca + cb - 1)
    return [(n, 2 * npoly, 0), (n, npoly, 1)]


def inverse_transforms(lb, L, npoly, inv_max):
    out, prev = [], 1
    if lb <= 1:
        return out
    for d in P.precision_sequence(L):
        if d + 1 > inv_max:
            n = P.next_pow_of_2(min(lb, d + 1) + 2 * prev - 2)
            out += [(n, 2 * npoly, 0), (n, npoly, 1)]
        prev = d + 1
    return out


def div_transforms(la, lb, npoly, mul_max, inv_max):
    L = la - lb + 1
    return inverse_transforms(lb, L, npoly, inv_max) + mul_transforms(la, L, L, npoly, mul_max)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "poly_time.jsonl")
    kzg = load_package()
    if kzg.device_count() < 1:
        raise SystemExit("time_poly.py: no GPU visible; nothing is measured without one")
    import torch

    rnd = random.Random(15)
    fs = kzg.FFTSettings(16)
    ps = kzg.PolySettings(fs)
    width, chunk, mul_max, inv_max = ps.info()
    T = kzg.PolySettings.transform_len
    # device buffers of the floor: the largest call transforms 2 x 16 lists of 2^16 elements
    cap = 2 * 16 * (1 << 16) * 32
    d_in = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")

    def floor_of(transforms):
        def run():
            for n, count, inv in transforms:
                fs.fft_fr_device(d_out.data_ptr(), d_in.data_ptr(), n, count, bool(inv))
            torch.cuda.synchronize()
        return run

    def rand_polys(n, npoly):
        return fr_bulk([rnd.randrange(1, R) for _ in range(n * npoly)])  # non-zero: any of them may lead or divide

    LA, LB = 1 << 15, 1 << 14
    a16, b16 = rand_polys(LA, 16), rand_polys(LB, 16)
    xs16 = rand_polys(16, 1)
    legs = []

    def leg(name, shape, call, transforms, want_len):
        assert max([t[0] for t in transforms], default=0) == want_len, (name, transforms, want_len)
        legs.append((name, shape, call, floor_of(transforms), transforms))

    for npoly in (1, 16):
        leg("div_%d" % npoly, {"la": LA, "lb": LB, "npoly": npoly}, lambda n=npoly: ps.div(a16, LA, b16, LB, n),
            div_transforms(LA, LB, npoly, mul_max, inv_max), T("div", LA, LB, 0))
    leg("mul_16k", {"la": LB, "lb": LB, "out_len": 2 * LB - 1, "npoly": 1}, lambda: ps.mul(a16, LB, b16, LB, 2 * LB - 1, 1),
        mul_transforms(LB, LB, 2 * LB - 1, 1, mul_max), T("mul", LB, LB, 2 * LB - 1))
    leg("inverse_16k1", {"lb": LB, "out_len": LB + 1, "npoly": 1}, lambda: ps.inverse(b16, LB, LB + 1, 1),
        inverse_transforms(LB, LB + 1, 1, inv_max), T("inverse", 0, LB, LB + 1))
    for nx in (1, 16):
        leg("eval_%d" % nx, {"len": LA, "npoly": 1, "nx": nx}, lambda k=nx: ps.eval(a16, LA, 1, xs16, k), [], 0)
    # sweeps
    for n in (8, 16, 32, 48, 64, 96, 128, 256, 1024):
        for form in (1, 2):
            leg("sweep_mul_%d_form%d" % (n, form), {"la": n, "lb": n, "out_len": 2 * n - 1, "npoly": 1, "form": form},
                lambda m=n, f=form: ps.mul(a16, m, b16, m, 2 * m - 1, 1, f), mul_transforms(n, n, 2 * n - 1, 1, mul_max, form),
                T("mul", n, n, 2 * n - 1) if form == 2 else 0)
    for L in (16, 32, 64, 128, 256):
        leg("sweep_inverse_%d" % L, {"lb": 40, "out_len": L, "npoly": 1}, lambda m=L: ps.inverse(b16, 40, m, 1),
            inverse_transforms(40, L, 1, inv_max), T("inverse", 0, 40, L))
    for lg in range(10, 16):
        leg("sweep_eval_%d" % (1 << lg), {"len": 1 << lg, "npoly": 1, "nx": 1}, lambda m=1 << lg: ps.eval(a16, m, 1, xs16, 1), [], 0)

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
            row = {"date": date, "row": name, **shape, "eval_chunk": chunk, "mul_direct_max": mul_max, "inv_direct_max": inv_max,
                   "transforms": [list(t) for t in transforms], "new": new, "transforms_alone": ref,
                   "difference_ms": round(new["median_ms"] - ref["median_ms"], 3)}
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
    ps.close()
    fs.close()


if __name__ == "__main__":
    main()
