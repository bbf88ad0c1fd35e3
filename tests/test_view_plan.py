"""view_plan.h's plan_views -- how rt_render_views cuts its views into launches of whole views -- built with g++ and checked
on the host (tests/native/view_plan_check.cpp): the cases worked out from its rules (5 views under a cap of two run as
2 + 2 + 1; V = 1; a cap of exactly one view; width * height * spp near 2^31) and its invariants over a sweep: the groups
are whole views in order and cover every view once, a group stays within kMaxPassSlots, the workspace budget and
views.max_paths, and a single view above kMaxPassSlots is refused."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_view_plan(tmp_path):
    exe = tmp_path / "view_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "another_raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "view_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
