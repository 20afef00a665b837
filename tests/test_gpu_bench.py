"""bench.py as every change is measured: a plain run (no --full) times exactly --steps steps, prints the headline line
without the side measurements, and --dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(dev, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
           "--dump-outputs", str(tmp_path)]
    pr = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert pr.returncode == 0, pr.stderr.decode()[-3000:]
    lines = [ln for ln in pr.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    assert j["steps"] == 4 and j["warmup"] == 2 and j["unit"] == "query-images/sec" and j["higher_is_better"] is True
    assert j["metric"].startswith("query-images/sec") and j["dtype"].startswith("f32")
    assert j["value"] > 0 and abs(j["value"] - 4 * 1000.0 / j["ms_per_step"]) < 1e-3 * j["value"] + 1e-2
    assert not set(j) & {"roofline", "train_step", "cpu_baseline", "eval_b1", "configs_1_cisa_only"}
    assert j["host_enqueue_ms_per_step"] is None
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert {"rois", "cls_prob", "bbox_pred", "rois_label", "RCNN_loss_cls"} <= set(got)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert got["rois"].shape[0] == 4 and got["rois"].shape[-1] == 5 and got["cls_prob"].shape[-1] == 2
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 * 10 ** 6
