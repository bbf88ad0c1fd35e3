"""call_plan.h -- the host decisions of a call on the caller's own buffers (rt_query_rays, rt_radiance_rays,
rt_render_views, rt_scene_update_triangles, rt_camera_rays; the frame calls' variant) -- built with g++ and checked on the
host (tests/native/call_plan_check.cpp): the eight rows of (device buffers, caller's stream, timed) for both rules, each
with its stream and whether the call waits, and the workspace's slot target."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_call_plan(tmp_path):
    exe = tmp_path / "call_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "another_raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "call_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
