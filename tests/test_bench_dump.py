"""bench.py --dump-outputs: the arrays the timed path computed in its last step, written so that two builds can be
compared output for output; and --steps is the number of timed steps."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_writes_float32_rows_exactly(tmp_path):
    b = _bench()
    com = np.random.default_rng(1).integers(0, 256, (300, 48), dtype=np.uint8)
    st = np.arange(300, dtype=np.int32) % 3
    b.dump_outputs(str(tmp_path), com, st)
    assert sorted(os.listdir(tmp_path)) == ["blob_index.npy", "commitments.npy", "status.npy"]
    got = {n: np.load(tmp_path / (n + ".npy")) for n in ("commitments", "status", "blob_index")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert (got["commitments"] == com).all() and (got["status"] == st).all() and (got["blob_index"] == np.arange(300)).all()


def test_dump_of_a_large_step_is_a_fixed_sample_under_64_mb(tmp_path):
    b = _bench()
    n = 400000  # 400 k blobs x 50 float32 = 80 MB unsampled
    com = (np.arange(n, dtype=np.uint32)[:, None] * 7 + np.arange(48, dtype=np.uint32)[None, :]).astype(np.uint8)
    st = np.zeros(n, dtype=np.int32)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), com, st, "_rank1")
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["blob_index_rank1.npy", "commitments_rank1.npy", "status_rank1.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    idx = np.load(tmp_path / "a" / "blob_index_rank1.npy").astype(np.int64)
    assert 0 < len(idx) < n and (np.diff(idx) > 0).all()
    assert (np.load(tmp_path / "a" / "commitments_rank1.npy") == com[idx]).all()
    for f in files:
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all(), f


def test_bench_refuses_zero_steps():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120, cwd=ROOT)
    assert p.returncode != 0
    assert "--steps must be at least 1" in p.stdout.decode()


@pytest.mark.gpu
def test_dump_holds_the_commitments_of_the_timed_path(kzg, oracle, oracle_settings, tmp_path):
    """A short bench run: the result line counts the steps it was given, and the dumped commitments of its last step
    are the oracle's commitments of the bench's own seeded blobs."""
    import ctypes as C

    import torch

    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "64", "--batches-per-step", "2", "--streams", "2", "--no-extras", "--no-counters",
                        "--no-cpu-baseline", "--no-multi", "--dump-outputs", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:]
    res = json.loads(out.strip().splitlines()[-1])
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    assert abs(res["ms_per_step"] - res["timed_region_s"] * 1e3 / 3) < 1e-6 * res["ms_per_step"]
    com = np.load(tmp_path / "commitments.npy")
    st = np.load(tmp_path / "status.npy")
    assert com.shape == (128, 48) and com.dtype == np.float32 and (st == 0).all()
    blobs = _bench().make_blobs(torch, 128, 4844, torch.device("cuda", 0)).cpu().numpy()
    for i in (0, 63, 64, 127):
        want = C.create_string_buffer(48)
        assert oracle.lib().oblob_to_kzg_commitment(want, blobs[i].tobytes(), C.byref(oracle_settings)) == 0
        assert bytes(com[i].astype(np.uint8)) == want.raw, i
