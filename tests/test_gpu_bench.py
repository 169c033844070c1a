"""bench.py end to end at a tiny size: a plain run prints only the headline line, `--dump-outputs` writes what the last timed
step computed, `--full` adds the roofline measured inside the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--batch", "2", "--size", "64", "--steps", "3", "--warmup", "1"]


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *TINY, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_headline_and_dumped_outputs(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "images/sec" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and abs(line["value"] - 2 * 1e3 / line["ms_per_step"]) <= 0.02 * line["value"]
    for k in ("roofline", "parity_mode", "similarity", "infer_mode", "cpu_baseline"):
        assert k not in line, k
    files = sorted(os.listdir(tmp_path))
    assert {"loss.npy", "weights_sample.npy", "grads_sample.npy"} <= set(files)
    total = 0
    for f in files:
        a = np.load(tmp_path / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    assert float(np.load(tmp_path / "loss.npy")) == pytest.approx(line["loss"], rel=1e-6)
    assert np.abs(np.load(tmp_path / "grads_sample.npy")).max() > 0


def test_full_run_adds_the_roofline():
    line = _bench("--full", "--no-cpu-baseline", "--no-extras", "--parity-steps", "0")
    assert line["steps"] == 3 and line["roofline"]["event_samples"] > 0
