"""bench.py on one GPU: a plain run prints the headline line and measures nothing beyond it; --full adds the blocks that take
runs of their own (here the profiled GEMM-roofline step and the optimizer update; the CPU baseline and clock probe are left out for time)."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def run_bench(*extra):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_headline_only():
    out = run_bench()
    assert out["metric"] == "images/sec/node SDXL-base 1024^2 bf16 fwd+bwd" and out["unit"] == "images/sec"
    assert out["higher_is_better"] is True and out["dtype"] == "bf16" and out["steps"] == 2 and out["warmup"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0 and 0 < out["loss"] < 1000
    assert out["roofline"] is None and out["optimizer"] is None and "clock" not in out and "cpu_baseline" not in out


def test_full_run_adds_roofline_and_optimizer():
    out = run_bench("--full", "--no-cpu-baseline", "--no-clock-probe")
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["roofline"]["achieved"] > 0 and out["roofline"]["launches_per_step"] > 0
    assert out["optimizer"]["ms_per_update"] > 0
    assert "clock" not in out and "cpu_baseline" not in out
