"""bench.py without --full prints the headline figure and nothing else; --full adds what the headline does not need."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _line(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "64", "--batches-per-step", "2", "--streams", "2", *extra],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:]
    return json.loads(out.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_roofline():
    plain = _line()
    full = _line("--full", "--no-extras", "--no-counters", "--no-cpu-baseline", "--no-multi")
    for res in (plain, full):
        assert all(k in res for k in HEADLINE)
        assert res["metric"] == "blob_to_kzg_commitment_per_s" and res["value"] > 0 and res["ms_per_step"] > 0
        assert res["steps"] == 2 and res["warmup"] == 1
    # the plain line carries no field that --full lacks, and none of the figures that take work of their own
    assert set(plain) <= set(full)
    for k in ("roofline", "valu", "counters", "cpu_baseline", "ntt", "msm_sweep", "in_process_multi"):
        assert k not in plain, k
    assert full["roofline"]["kernel"] and full["roofline"]["kernel_ms"] > 0
