"""bench.py without --full: set up, warm up, time the steps, print -- the headline keys and nothing of the legs behind --full
(per-kernel roofline, PMC traffic, extras, parity, CPU baseline).  A small batch keeps it to seconds."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_only(dev, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "3", "--batch", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "fp16" and d["full"] is False
    assert d["value"] > 0 and d["ms_per_step"] > 0 and abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["graph_captures_in_timed_region"] == 0
    assert d["exchange"]["rows_gathered"] == 2 and d["exchange"]["regions_gathered"] == 200
    assert set(d["roofline"]) == {"bound", "peak", "unit", "e2e_algorithmic_tflops_per_gpu", "e2e_frac_of_peak"}
    assert not {"extras", "extras_summary", "parity", "cpu_baseline", "summary_tail"} & set(d)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in d["dump_outputs"]["arrays"])
