"""bench.py's command line on the GPU at a small size (256x128): a plain run times exactly --steps
steps, leaves the fields of --full null and writes its outputs with --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_outputs(tmp_path):
    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--height", "128", "--width", "256", "--dump-outputs", out]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "images/s" and line["higher_is_better"]
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: 2 images per step (both rounded to 3 decimals)
    assert line["value"] == pytest.approx(2e3 / line["ms_per_step"], rel=1e-3)
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["loss_delta_vs_cpu"] is None
    names = sorted(os.listdir(out))
    assert names == sorted(n + ".npy" for n in ("loss_seg", "loss_target", "state_sample", "conv1.weight",
                                                "layer3.5.conv2.weight", "layer6.conv2d_list.0.weight"))
    total = 0
    for n in names:
        x = np.load(os.path.join(out, n), allow_pickle=False)
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        total += x.nbytes
    assert total <= 64 * 1024 * 1024
    assert np.load(os.path.join(out, "loss_seg.npy")).shape == ()
    assert np.load(os.path.join(out, "conv1.weight.npy")).shape == (64, 3, 7, 7)
    assert np.load(os.path.join(out, "state_sample.npy")).std() > 0
