"""bench.py's plain run and its --dump-outputs: the line carries the headline only, the dump holds what the last timed step
handed its caller, and two runs with the same arguments dump the same bits (the inputs are seeded, the step has no atomics)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--patch", "32",
           "--batch", "2", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {n: np.load(os.path.join(out_dir, n + ".npy")) for n in ("loss", "params", "grads")}


def test_plain_bench_line_and_dumped_outputs_repeat(tmp_path):
    rec, a = _bench(tmp_path / "a")
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["unit"] == "patches/s"
    assert abs(rec["value"] - 2 * 1e3 / rec["ms_per_step"]) <= 1e-2 * rec["value"]
    for key in ("roofline", "roofline_wgrad", "fp32_parity_mode", "fp16_mode", "cpu_baseline", "cfg1_plumbing"):
        assert key not in rec, key  # behind --full
    assert a["loss"].shape == () and abs(float(a["loss"]) - rec["config"]["loss"]) <= 1e-6
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name, v in a.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), name
    assert np.abs(a["grads"]).max() > 0
    _, b = _bench(tmp_path / "b")
    for name in a:
        assert np.array_equal(a[name], b[name]), name
