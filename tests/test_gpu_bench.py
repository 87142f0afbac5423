"""bench.py on the device (pytest -m gpu): a plain run prints the headline line only and --dump-outputs writes the arrays of steps on
the seeded initial scene, the same in every run up to rounding; --full adds the measurements beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
BESIDE = {"stage_ms", "roofline", "rasterize_fwd_bwd_ms", "sync_free"}


def _line(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "GSR_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--P", "20000", "--W", "640",
                        "--H", "368", "--clock-prewarm-ms", "0"] + extra, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(tmp_path):
    d = _line(["--variant", "plane", "--dump-outputs", str(tmp_path)])
    assert HEADLINE <= set(d) and not BESIDE & set(d)
    assert d["steps"] == 3 and d["value"] > 0 and abs(d["ms_per_step"] - 1e3 / d["value"]) < 1e-3 * d["ms_per_step"] + 1e-3
    # the same command again: the dump has the same inputs, so it agrees up to the rounding of the float-atomic accumulation order --
    # outputs and gradients to ~1e-7 of their largest element; a parameter whose gradient is zero up to rounding can take Adam's +-lr
    # step (eps 1e-15) with either sign, so parameters are held to 2 lr per dumped step
    again = tmp_path.parent / (tmp_path.name + "_again")
    _line(["--variant", "plane", "--dump-outputs", str(again)])
    assert sorted(os.listdir(again)) == sorted(os.listdir(tmp_path))
    for n in os.listdir(tmp_path):
        a, b = np.load(tmp_path / n).astype(np.float64), np.load(again / n).astype(np.float64)
        tol = 2 * bench.DUMP_STEPS * bench.LEARNING_RATES[n[len("param_"):-4]] if n.startswith("param_") else 4e-6 * np.abs(a).max()
        assert a.shape == b.shape and np.abs(a - b).max() <= tol, (n, np.abs(a - b).max(), np.abs(a).max())
    assert np.array_equal(np.load(tmp_path / "out_radii.npy"), np.load(again / "out_radii.npy"))
    names = sorted(os.listdir(tmp_path))
    assert {"out_loss.npy", "out_color.npy", "out_radii.npy", "out_all_map.npy", "out_plane_depth.npy", "out_viewspace_grad.npy",
            "param_means3D.npy", "param_colors_precomp.npy"} <= set(names)
    total = 0
    for n in names:
        a = np.load(tmp_path / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "out_color.npy").shape == (3, 368, 640) and (np.load(tmp_path / "out_radii.npy") > 0).any()


def test_full_run_adds_the_measurements_beside_the_headline():
    d = _line(["--full", "--no-cpu-baseline", "--no-method-iteration", "--no-graph-replay"])
    assert HEADLINE <= set(d) and BESIDE <= set(d)
    assert d["roofline"]["avg_launch_ms"] > 0 and d["config"]["tile_instances_R"] > 0
