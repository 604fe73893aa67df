#!/usr/bin/env python3
"""Generic polynomial KZG (kzgamd_kzg_commit / _open / _check) at the reference's bench shape — scale 15, 2^15
coefficients (bench_commit_to_poly / bench_compute_proof_single, kzg-bench/src/benches/kzg.rs) — beside the MSM-only
floor of any path that computes its quotients on the host: mult_pippenger_prepared / mult_pippenger_prepared_batch on a
handle over the same points with the same table budget, fed PRECOMPUTED quotients in the same batch counts.  The
difference between a call and its floor is what the upload of the polynomial and the quotient kernels cost.

  commit          kzgamd_kzg_commit, one polynomial                     floor: 1 MSM of 2^15
  open_1x1        kzgamd_kzg_open, n = 1, 1 point (ys wanted)           floor: 1 MSM of 2^15 - 1
  open_1x16       n = 1, 16 points                                      floor: 16 MSMs of 2^15 - 1 in one batch
  open_64x16      n = 64, 16 points                                     floor: 16 MSMs of 2^15 - 64 in one batch
  check_64x16     kzgamd_kzg_check, n = 64, 16 tuples; host_side = the G2 work and the pairings of the same tuples
                  alone, through the library's host helpers (kzgamd_p2_mult / _p2_add / kzgamd_pairings_verify)
  check_batch_NxC kzgamd_kzg_check_batch (derived r), n = 64 with 16 / 256 / 4096 tuples and n = 1 with 16 / 4096, beside
                  kzgamd_kzg_check on the same tuples (up to 256) in the same loop; and its stages, each timed alone:
                  hash = kzgamd_kzg_batch_challenge, g1_sides = kzgamd_kzg_check_batch_g1 with a given r (everything on
                  the GPU), given_r = kzgamd_kzg_check_batch with a given r (g1_sides + the pairing)

One process, legs alternating, after warm-up; host clock around synchronous calls (every entry point returns when its
output is in host memory), as tools/time_fk20.py.  The setup points are [i + 1]G (valid G1 points; the time does not
depend on their values), so the check's verdicts are not meaningful here — tests/test_kzg_gpu.py checks values.  One
JSON line per row (median and spread = max - min of `reps` runs, ms), appended to the output file.
python tools/time_kzg.py [reps] [table_budget_gb] [output.jsonl]"""
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
import kzg_model as M
import oracle_ffi as O
from conftest import load_package

R = O.R
LEN = 1 << 15


def setup_points(n):
    L = O.lib()
    jac, aff = (O.G1 * n)(), (O.G1Affine * n)()
    cur, g = O.G1(), O.G1()
    L.og1_generator(C.byref(g))
    C.memmove(C.byref(cur), C.byref(g), 144)
    for i in range(n):
        C.memmove(C.byref(jac[i]), C.byref(cur), 144)
        L.og1_to_affine(C.byref(aff[i]), C.byref(cur))
        nxt = O.G1()
        L.og1_add_or_dbl(C.byref(nxt), C.byref(cur), C.byref(g))
        cur = nxt
    return jac, aff


def fr_bulk(vals):
    raw = b"".join(((v << 256) % R).to_bytes(32, "little") for v in vals)
    arr = (O.Fr * max(1, len(vals)))()
    C.memmove(arr, raw, len(raw))
    return arr


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "spread_ms": round(max(ts) - min(ts), 3), "runs": len(ts)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    budget_gb = float(sys.argv[2]) if len(sys.argv) > 2 else 40.0
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "kzg_time.jsonl")
    kzg = load_package()
    if kzg.device_count() < 1:
        raise SystemExit("time_kzg.py: no GPU visible; nothing is measured without one")
    rnd = random.Random(15)
    jac, aff = setup_points(LEN)
    g2gen = kzg.p2_generator()
    g2 = (kzg.BlstP2 * 65)()
    s = 0x1234567
    for i in range(65):
        g2[i] = kzg.p2_mult(g2gen, fr_bulk([pow(s, i, R)])[0])
    fs = kzg.FFTSettings(15)
    cfg = kzg.make_config(table_budget_gb=budget_gb)
    kz = kzg.PolyKZGSettings(fs, jac, LEN, g2, 65, cfg)
    floor = kzg.prepare_multi_scalar_mult(aff, LEN, kzg.make_config(table_budget_gb=budget_gb))
    p = [rnd.randrange(R) for _ in range(LEN)]
    xs = [rnd.randrange(1, R) for _ in range(16)]
    fp, fx = fr_bulk(p), fr_bulk(xs)
    quot = {n: fr_bulk([c for x in xs for c in M.long_division(p, n, pow(x, n, R))[0]]) for n in (1, 64)}
    # the check's inputs: real proofs and values of this polynomial (the verdicts are not looked at, see above)
    proofs64, ys64 = kz.open(fp, LEN, 1, fx, 16, 64)
    com = kz.commit(fp, LEN)
    com16 = (kzg.BlstP1 * 16)()
    for i in range(16):
        C.memmove(C.byref(com16[i]), com, 144)

    def host_side():
        for i in range(16):
            xn = kzg.p2_mult(g2gen, fr_bulk([R - pow(xs[i], 64, R)])[0])
            rhs = kzg.p2_add(g2[64], xn)
            kzg.pairings_verify(com16[i], g2gen, proofs64[i], rhs)

    legs = [
        ("commit", lambda: kz.commit(fp, LEN), lambda: kzg.multi_scalar_mult_prepared(floor, fp, LEN)),
        ("open_1x1", lambda: kz.open(fp, LEN, 1, fx, 1, 1), lambda: kzg.multi_scalar_mult_prepared(floor, quot[1], LEN - 1)),
        ("open_1x16", lambda: kz.open(fp, LEN, 1, fx, 16, 1),
         lambda: kzg.multi_scalar_mult_prepared_batch(floor, quot[1], LEN - 1, 16)),
        ("open_64x16", lambda: kz.open(fp, LEN, 1, fx, 16, 64),
         lambda: kzg.multi_scalar_mult_prepared_batch(floor, quot[64], LEN - 64, 16)),
        ("check_64x16", lambda: kz.check(com16, proofs64, fx, ys64, 64, 16), host_side),
    ]
    for _, new, ref in legs:  # warm-up: code objects, workspaces, line tables
        new()
        ref()
        new()
        ref()
    runs = {name: ([], []) for name, _, _ in legs}
    for _ in range(reps):
        for name, new, ref in legs:
            t0 = time.perf_counter()
            new()
            t1 = time.perf_counter()
            ref()
            t2 = time.perf_counter()
            runs[name][0].append((t1 - t0) * 1e3)
            runs[name][1].append((t2 - t1) * 1e3)
    info = kz.info()
    date = datetime.date.today().isoformat()
    with open(out_path, "a") as f:
        for name, _, _ in legs:
            new, ref = stats(runs[name][0]), stats(runs[name][1])
            second = "host_side" if name.startswith("check") else "msm_floor"
            row = {"date": date, "row": name, "len": LEN, "table_budget_gb": budget_gb, "chunk": info[2], "lane_form_min": info[3],
                   "wide_table": int(kzg.lib().kzgamd_msm_uses_wide_table(floor.handle)), "new": new, second: ref,
                   "difference_ms": round(new["median_ms"] - ref["median_ms"], 3)}
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
    batch_rows(kzg, kz, fp, rnd, reps, budget_gb, out_path, date)
    kz.close()
    floor.close()
    fs.close()


def batch_rows(kzg, kz, fp, rnd, reps, budget_gb, out_path, date):
    """check_batch beside the per-tuple check on the same tuples: 256 openings of the polynomial per n, repeated to 4096"""
    base = 256
    xs = [rnd.randrange(1, R) for _ in range(base)]
    fx = fr_bulk(xs)
    com = bytes(kz.commit(fp, LEN))[:144]
    with open(out_path, "a") as f:
        for n, counts in ((64, (16, 256, 4096)), (1, (16, 4096))):
            proofs, ys = kz.open(fp, LEN, 1, fx, base, n)
            proofs, ys, xraw = bytes(proofs)[:144 * base], bytes(ys)[:32 * n * base], bytes(fx)[:32 * base]
            for count in counts:
                rep = -(-count // base)
                c, p_, x_, y_ = com * count, (proofs * rep)[:144 * count], (xraw * rep)[:32 * count], (ys * rep)[:32 * n * count]
                r = kzg.batch_challenge(c, p_, x_, y_, n, count)
                legs = [("new", lambda: kz.check_batch(c, p_, x_, y_, n, count)),
                        ("hash", lambda: kzg.batch_challenge(c, p_, x_, y_, n, count)),
                        ("g1_sides", lambda: kz.check_batch_g1(c, p_, x_, y_, n, count, r=r)),
                        ("given_r", lambda: kz.check_batch(c, p_, x_, y_, n, count, r=r))]
                if count <= 256:
                    legs.append(("per_tuple_check", lambda: kz.check(c, p_, x_, y_, n, count)))
                kz.check_batch(c, p_, x_, y_, n, count)  # warm-up: workspaces, the line table of [s^n]G2
                for _, fn in legs:
                    fn()
                ts = {name: [] for name, _ in legs}
                for _ in range(reps):
                    for name, fn in legs:
                        t0 = time.perf_counter()
                        fn()
                        ts[name].append((time.perf_counter() - t0) * 1e3)
                row = {"date": date, "row": "check_batch_%dx%d" % (n, count), "len": LEN, "table_budget_gb": budget_gb}
                row.update({name: stats(v) for name, v in ts.items()})
                line = json.dumps(row)
                print(line, flush=True)
                f.write(line + "\n")


if __name__ == "__main__":
    main()
