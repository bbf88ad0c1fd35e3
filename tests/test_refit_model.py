"""refit.h -- the arithmetic rt_scene_update_triangles' kernels share with the BVH builder -- built with g++ and checked on the
host (tests/native/refit_check.cpp): conservative_box against an independent restatement (long-double compares and
nextafterf) over doubles that are floats, one f64 ulp either side of a float, negative, +-1e30, 1e-30 and 0 -- the box
contains the interval and its bits are the documented formula's; a host model of the level refit on a hand-made
three-level node array with an empty slot and a four-primitive leaf -- every box contains the f64 boxes below it and is
the specified one, the level table is contiguous and children lie below their parents; and the primitive boxes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_refit_model(tmp_path):
    exe = tmp_path / "refit_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "another_raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "refit_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
