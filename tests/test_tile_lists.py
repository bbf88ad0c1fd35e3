"""tile_lists.h -- which spheres the camera rays of an 8x8 tile can reach, the test behind k_paths' per-tile sphere lists
-- built with g++ and checked on the host against brute force (tests/native/tile_lists_check.cpp): rays formed as cam_ray
forms them, with s, t and the lens offset at random and at their extremes, must hit candidates only.  The cases: the
benchmark-like layout at 1920x1080 (sampled tiles) and 72x40 (partial tiles), aperture 0 and 2, the camera inside a
sphere, a sphere straddling the lens plane and one behind the camera, moving spheres, band_rows 4 with three bands, and a
sphere tangent to a bundle's edge.  On the 1080p layout no tile overflows the record's 15 slots and the mean count is
below 4: the precondition of the speed-up."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_tile_lists(tmp_path):
    exe = tmp_path / "tile_lists_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "another_raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "tile_lists_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "ok", out.stdout
