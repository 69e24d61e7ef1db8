"""bench.py's plain run measures the headline and nothing else: the side figures, the CPU baseline and the rocprofv3 child
passes run with --full alone (tests/test_decode_world2_gpu.py runs --full at N > 1)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_FIGURES = {"fused_launches_figure", "decode_1gpu", "fakequant_block", "config5", "cpu_baseline", "decode_pipeline"}


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "TFLOP/s" and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert not SIDE_FIGURES & set(d), sorted(SIDE_FIGURES & set(d))
    assert "traffic_by_shape" not in d["roofline"] and d["roofline"]["achieved"] > 0
