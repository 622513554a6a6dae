"""-m gpu: what `bench.py` prints at N = 1 on a small scene - a plain run the headline alone, `--full` everything else beside it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gaussians", "20000", "--width", "320", "--height", "200", "--cameras", "8", "--steps", "4", "--warmup", "2"]
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
            "config"}


def _bench(*args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + SMALL + list(args), cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_alone(tmp_path):
    out = _bench("--dump-outputs", str(tmp_path))
    assert set(out) == HEADLINE
    assert out["steps"] == 4 and out["warmup"] == 2 and out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert out["config"]["frames_redone"] == 0 and out["config"]["discarded_region_frames_per_s"] > 0
    image = np.load(os.path.join(str(tmp_path), "image.npy"))
    assert image.shape == (3, 200, 320) and np.isfinite(image).all()
    assert np.load(os.path.join(str(tmp_path), "radii.npy")).shape == (20000,)
    assert np.load(os.path.join(str(tmp_path), "num_rendered.npy"))[0] > 0


def test_full_run_adds_the_other_measurements():
    out = _bench("--full", "--no-c5", "--repeats", "1")
    assert HEADLINE <= set(out)
    assert len(out["repeats"]["frames_per_s"]) == 1 and set(out["variants"]) >= {"backward_state", "cov9"}
    assert out["single_stream"]["ms_per_frame"] > 0 and out["stage_ms"]["render"] > 0 and out["roofline"]["avg_ms"] > 0
    assert out["frame_roofline"]["algorithmic_bytes"] > 0 and out["batch"]["frames_per_launch"] == 4
    assert out["fwd_bwd"]["ms_per_iter"] > 0 and out["fwd_bwd"]["c2_500k_ms_per_iter"] > 0 and out["fwd_bwd"]["ms_per_training_iteration"] > 0
    assert out["cpu_baseline"]["value"] > 0
    assert "c5" not in out
