"""bench.py: a plain run does only what its headline needs; the legs that run work of their own come with --full."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _line(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--n-utts", "512"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_has_no_side_legs_and_full_adds_them():
    assert torch.cuda.is_available(), "gpu-marked test needs a HIP device"
    plain = _line([])
    assert all(k in plain for k in HEADLINE) and plain["value"] > 0 and plain["steps"] == 3 and plain["warmup"] == 2
    for k in ("roofline", "cpu_baseline"):
        assert k not in plain
    for k in ("host_fed_ms_per_step", "x_over_cpu", "other_configs"):
        assert k not in plain["config"]
    # --full, the CPU baseline and the other configurations dropped as single legs: host-fed steps and the roofline replay
    full = _line(["--full", "--cpu-seconds", "0", "--no-other-configs"])
    assert all(k in full for k in HEADLINE) and full["value"] > 0
    assert full["roofline"]["kernel"] and full["config"]["host_fed_ms_per_step"] > 0
    assert "cpu_baseline" not in full and "other_configs" not in full["config"]
    # the same timed batches either way
    assert full["config"]["global_batch_mel_frames"] == plain["config"]["global_batch_mel_frames"]
