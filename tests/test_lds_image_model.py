"""lds_image.h -- the arithmetic rt_scene_update_spheres' kernels share with the LDS scene image's builder -- built with
g++ and checked on the host (tests/native/lds_image_check.cpp): image_put_sphere and image_put_node_boxes against literal
expectations for a static sphere, a moving sphere with c = -0.0 and d = +0.0 (the image stores c + d = +0.0), a node
with an empty child and a node updated twice; neither writes a byte outside the planes it owns."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lds_image_model(tmp_path):
    exe = tmp_path / "lds_image_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "another_raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "lds_image_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
