"""pass_plan.h's path_chunk -- how many path slots a persistent kernel's wave claims per atomic on the pass counter
(k_paths.hip k_paths / k_paths_g.h k_paths_g; r4r_ab_path_chunk.txt) -- built with g++ and checked on the host: its values at the
BASELINE configs' pass sizes and its invariants (a power of two in [64, 2048], monotone in the pass size, at least 64
claims per wave of a full CU above the minimum)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_path_chunk(tmp_path):
    exe = tmp_path / "pass_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "another_raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "pass_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pass_plan(tmp_path):
    """plan_passes (samples per pass and pass count: the kMaxPassSlots clamp, the even spread of rt_render, none for the
    noise-target base pass), list_pass_samples and round_pass_samples: the cases worked out from the renderer's rules
    (1920x1080 at 2100 spp with samples_per_pass 2100 -> 3 passes of 700) and the invariants k >= 1,
    k * npix_pad <= 2^31, npasses * k >= spp > (npasses - 1) * k over a sweep."""
    exe = tmp_path / "pass_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "another_raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "pass_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), "plan"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
