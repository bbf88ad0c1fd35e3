"""bench.py's output contract on a small frame (the driver parses this line at round end): one JSON line with the
metric, value, unit, n_gpus, steps, warmup, ms_per_step, higher_is_better, scaling, vs_baseline, dtype, data and
config fields, plus the roofline object of the dominant kernel; value = segments / wall time.  A plain run stops
there (no cpu_baseline, no parity: those take runs of their own and belong to --full); --dump-outputs writes the last
timed step's frame and counts, the same arrays on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--width", "96", "--height", "54", "--spp", "8",
                          "--steps", "2", "--warmup", "1", *args], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("scene,variant,kernel", [("1", 3, "k_paths"), ("cow", 4, "k_paths_g")])
def test_bench_line_contract(gpu, tmp_path, scene, variant, kernel):
    d = _bench("--scene", scene, "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "out"))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert "cpu_baseline" not in d and "parity" not in d  # a plain run: only what the headline figure needs
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["unit"] == "Msamples/s" and d["value"] > 0
    c = d["config"]
    assert (c["width"], c["height"], c["spp"]) == (96, 54, 8) and c["primary_rays_per_step"] == 96 * 54 * 8
    assert c["segments_per_step"] >= c["primary_rays_per_step"]
    # value is the whole job's segments over the timed wall time
    assert d["value"] == pytest.approx(c["segments_per_step"] * d["steps"] / (d["ms_per_step"] * d["steps"] * 1e3), rel=2e-3)
    assert c["driver"] == "multi" and "rt_render_multi" in c["parallelism"]
    r = d["roofline"]
    assert r["kernel"] == kernel and r["extend_variant"] == variant and r["launches"] == 2 and r["devices"] == 1
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["avg_launch_ms"] > 0
    # achieved = the algorithmic bytes of one launch over its measured duration
    assert r["achieved"] == pytest.approx(r["algorithmic_bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9, rel=1e-3)
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-3, abs=1e-6)
    assert r["segments_per_launch"] == c["segments_per_step"]
    # the dumped outputs: the last timed step's RGB8 frame (the oracle's, bit for bit) and its exact counts
    from tests.oracle_lib import oracle_render
    frame = np.load(tmp_path / "out" / "frame.npy")
    stats = np.load(tmp_path / "out" / "stats.npy")
    assert sorted(os.listdir(tmp_path / "out")) == ["frame.npy", "stats.npy"]
    assert frame.dtype == np.float32 and frame.shape == (54, 96, 3) and stats.dtype == np.float64
    ref = oracle_render(scene, 96, 54, 8, mode="pcg", seed=0)
    assert np.array_equal(frame, ref["rgb"].astype(np.float32))
    assert stats.tolist() == [c["segments_per_step"], c["primary_rays_per_step"]] and stats[0] == ref["segments"]


@pytest.mark.gpu
def test_bench_full_adds_parity(gpu):
    # --full: the same line plus the checks that run after the timed steps (the CPU baselines are dropped here: they
    # take minutes at any frame size worth timing)
    d = _bench("--scene", "1", "--full", "--no-cpu-baseline")
    assert "roofline" in d and "cpu_baseline" not in d
    p = d["parity"]
    assert p["bit_exact"] is True and p["max_dlsb"] == 0 and p["spp"] == 8 and p["pixels"] == len(p["rows"]) * 96
