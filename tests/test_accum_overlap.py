"""pass_plan.h's split_pass -- whether and where a planned whole-image k_paths pass is cut into a head and a tail launch
so that the head's sums run while the tail traces (option render.accum_overlap) -- built with g++ and checked on the
host (tests/native/accum_overlap_check.cpp); the option's range and default through the C ABI."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_split_pass(tmp_path):
    exe = tmp_path / "accum_overlap_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "another_raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "accum_overlap_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout


def test_option_range_and_default():
    import another_raytracer_amd as art
    assert art.get_option("render.accum_overlap") == 1  # auto
    try:
        for v in (0, 2, 1):
            art.set_option("render.accum_overlap", v)
            assert art.get_option("render.accum_overlap") == v
        for bad in (-1, 3, 0.5):
            with pytest.raises(art.RTError):
                art.set_option("render.accum_overlap", bad)
    finally:
        art.set_option("render.accum_overlap", 1)
