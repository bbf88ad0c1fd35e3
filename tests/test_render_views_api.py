"""rt_render_views: the argument checks (every refusal happens before a device is touched, with a message), the export and
its binding, option views.max_paths, the Python wrapper's buffer checks, the C++ facade and the new kernels' register
budgets.  Host-only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import (RT_ADAPTIVE, RT_GLOBAL_SCENE, RT_OUT_DEVICE, RT_PARALLEL_IMAGES, RT_PROFILE, RT_SPLIT_SHADE, RT_WAVEFRONT, lib,
                                        rt_camera, rt_params, rt_stats)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

RT_OK, RT_E_INVALID, RT_E_DEVICE = 0, -1, -3
V, W, H = 3, 16, 9


@pytest.fixture(scope="module")
def world():
    return art.scene_manager().build("c1")


def _call(world, nviews=V, scene=True, cams=True, params=True, rgb=True, accum=False, seeds=False, stats=False, **fields):
    table = (rt_camera * V)(*[rt_camera((0, 0, 5 + v), (0, 0, 0), (0, 1, 0), 40.0, W / H, 0.0, 5.0, 0.0, 1.0) for v in range(V)])
    p = rt_params(width=W, height=H, spp=2, max_depth=50, band_rows=H, band_count=1)
    for k, v in fields.items():
        setattr(p, k, v)
    out = np.zeros((V, H, W, 3), np.uint8)
    acc = np.zeros((V, H, W, 3), np.float64)
    seed_arr = (ctypes.c_uint64 * V)(1, 2, 3)
    st = rt_stats()
    return lib.rt_render_views(world.objects._native if scene else None, table if cams else None, seed_arr if seeds else None, nviews,
                               ctypes.byref(p) if params else None, out.ctypes.data_as(ctypes.c_void_p) if rgb else None,
                               acc.ctypes.data_as(ctypes.c_void_p) if accum else None, ctypes.byref(st) if stats else None)


def _refused(world, **kw):
    return _call(world, **kw) == RT_E_INVALID and len(lib.rt_last_error()) > 0


def test_the_symbol_is_exported_and_bound():
    nm = subprocess.run(["nm", "-D", "--defined-only", art._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T rt_render_views\n" in nm
    assert "rt_render_views" in art._lib.SIGNATURES and callable(art.render_views) and "render_views" in art.__all__
    assert lib.rt_abi_version() == 5  # the addition is additive


def test_null_arguments_are_refused(world):
    assert _refused(world, scene=False)
    assert _refused(world, cams=False)
    assert _refused(world, params=False)
    assert _refused(world, rgb=False)          # out_rgb8 NULL with nviews > 0
    assert _refused(world, nviews=-1)
    assert _refused(world, nviews=-(1 << 31))


def test_parameters_outside_their_range_are_refused(world):
    assert _refused(world, width=1)
    assert _refused(world, height=1)
    assert _refused(world, width=0)
    assert _refused(world, spp=0)
    assert _refused(world, spp=-3)
    assert _refused(world, max_depth=0)
    assert _refused(world, max_depth=-1)
    assert _refused(world, fp_mode=1)
    assert _refused(world, stream=1234)                        # a stream without RT_OUT_DEVICE
    assert _refused(world, band_count=2)                       # the whole frame only
    assert _refused(world, band_count=0)
    assert _refused(world, band_count=2, band_index=1, band_rows=3)
    assert _refused(world, band_count=1, band_index=1)


@pytest.mark.parametrize("flag", [RT_PROFILE, RT_SPLIT_SHADE, RT_ADAPTIVE, RT_WAVEFRONT, RT_PARALLEL_IMAGES, 128, 256, 512, 1024, 1 << 30])
def test_other_flag_bits_are_refused(world, flag):
    assert _refused(world, flags=flag)
    assert _refused(world, flags=flag | RT_OUT_DEVICE | RT_GLOBAL_SCENE)


def test_a_view_above_the_launch_limit_is_refused_and_pointed_at_rt_render(world):
    # 32768 x 32768 x 3 samples > 2^31 paths in one view; x 2 is exactly the limit and passes the check (it then needs a device)
    assert _refused(world, width=32768, height=32768, spp=3)
    assert b"kMaxPassSlots" in lib.rt_last_error() and b"rt_render" in lib.rt_last_error()
    assert _refused(world, width=65536, height=32768, spp=2)
    assert _refused(world, width=2, height=2, spp=(1 << 29) + 1)
    assert _refused(world, nviews=0, width=32768, height=32768, spp=3)  # the parameters are checked before the count


@pytest.mark.parametrize("fields", [{}, {"flags": RT_OUT_DEVICE}, {"flags": RT_GLOBAL_SCENE, "spp": 8}, {"flags": RT_OUT_DEVICE, "stream": 1234}])
def test_zero_views_is_ok_and_touches_no_device(world, fields):
    # no device on a host-only machine: RT_OK shows the call returned before any device work
    assert _call(world, nviews=0, **fields) == RT_OK
    assert _call(world, nviews=0, rgb=False, stats=True, seeds=True, **fields) == RT_OK
    assert art.render_views(world, [], W, H, 2).shape == (0, H, W, 3)


@pytest.mark.skipif(lib.rt_device_count() > 0, reason="checks the no-device failure path")
def test_a_valid_call_without_a_device_fails_loudly(world):
    assert _call(world) == RT_E_DEVICE  # the arguments passed every check
    assert _call(world, seeds=True, accum=True, stats=True) == RT_E_DEVICE
    assert _call(world, nviews=1, spp=1, max_depth=1) == RT_E_DEVICE
    assert _call(world, band_rows=0) == RT_E_DEVICE            # band_rows is not read
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0)
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.render_views(world, [cam, cam], W, H, 2, seeds=[1, 2], accum=True, stats=True)


def test_the_option_round_trips(world):
    assert art.get_option("views.max_paths") == 0  # off
    try:
        art.set_option("views.max_paths", 7680)
        assert art.get_option("views.max_paths") == 7680
        art.set_option("views.max_paths", 1 << 31)
        assert art.get_option("views.max_paths") == float(1 << 31)
        for bad in (-1, 0.5, (1 << 31) + 1):
            with pytest.raises(art.RTError, match="RT_E_INVALID"):
                art.set_option("views.max_paths", bad)
        assert art.get_option("views.max_paths") == float(1 << 31)
        art.set_option(None, 0)  # reset every option
        assert art.get_option("views.max_paths") == 0
    finally:
        art.set_option("views.max_paths", 0)


def test_python_wrapper_refuses_wrong_buffers_and_arguments(world):
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0)
    cams = [cam, cam]
    for bad in (np.zeros((2, H, W, 3), np.int8), np.zeros((2, H, W, 4), np.uint8), np.zeros((1, H, W, 3), np.uint8), np.zeros((2, W, H, 3), np.uint8),
                np.zeros((2, H, W, 6), np.uint8)[..., ::2], np.zeros(2 * H * W * 3, np.uint8)):
        with pytest.raises(ValueError):
            art.render_views(world, cams, W, H, 2, out=bad)
    for bad in (np.zeros((2, H, W, 3), np.float32), np.zeros((2, H, W), np.float64), np.zeros((3, H, W, 3), np.float64)):
        with pytest.raises(ValueError):
            art.render_views(world, cams, W, H, 2, accum=bad)
    with pytest.raises(TypeError):
        art.render_views(world, cams, W, H, 2, out=[0] * (2 * H * W * 3))
    with pytest.raises(ValueError):
        art.render_views(world, cams, W, H, 0)
    with pytest.raises(ValueError):
        art.render_views(world, cams, W, H, 2, seeds=[1])          # one seed per camera
    with pytest.raises(ValueError):
        art.render_views(world, cams, W, H, 2, stream=1234)        # a stream belongs to device tensors
    with pytest.raises(TypeError):
        art.render_views(world, [cam, None], W, H, 2)
    with pytest.raises(TypeError):
        art.render_views(art.hittable_list(), cams, W, H, 2)       # not compiled
    with pytest.raises(TypeError):
        art.render_views(None, cams, W, H, 2)
    import torch
    with pytest.raises(ValueError):
        art.render_views(world, cams, W, H, 2, out=torch.zeros((2, H, W, 3), dtype=torch.uint8))   # a tensor, but on the host
    with pytest.raises(ValueError):
        art.render_views(world, cams, W, H, 2, out=np.zeros((2, H, W, 3), np.uint8), accum=torch.zeros((2, H, W, 3), dtype=torch.float64))


def test_the_cpp_facade_compiles(tmp_path):
    src = tmp_path / "q.cpp"
    src.write_text("""
#include "art_engine.hpp"
int main() {
    art::scene_manager sm("assets");
    art::scene world = sm.build("6");
    const int W = 16, H = 9;
    std::vector<art::camera> cams;
    for (int v = 0; v < 3; ++v)
        cams.emplace_back(art::point3{{0.0, 1.0 + v, 5.0}}, world.lookat, art::vec3{{0, 1, 0}}, world.vfov, 16.0 / 9.0, world.aperture, 10.0, 0.0, 1.0);
    std::vector<std::uint8_t> rgb(3 * W * H * cams.size());
    std::vector<double> sums(3 * W * H * cams.size());
    art::views_options o;
    o.spp = 4;
    o.max_depth = 20;
    o.background = world.background;
    rt_stats st{};
    art::render_views(world, cams, W, H, rgb.data());
    art::render_views(world, cams, W, H, rgb.data(), o, {7, 8, 9}, sums.data(), &st);
    return st.passes == 1 && st.segments >= st.primary ? 0 : 1;
}
""")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_view_kernels_are_no_worse_than_their_memory_source_siblings():
    """The nine k_radiance_views forms against DESIGN.md 4.8's figures for k_radiance_rays: the LDS-image form within one
    1024-lane block's 128 VGPRs and no spill, the HBM-scene forms within three waves' 168 VGPRs, and no form spilling more
    than its sibling (0, but the three all-features forms: 2 / 3 / 3).

    Measured on the built code object: VGPRs 128; 129 / 147; 152 / 156 / 157; 168 / 168 / 168 with 0 / 3 / 3 spilled.
    """
    ks = kernel_resources.kernels(os.path.join(ROOT, "another_raytracer_amd", "libart.so"))
    views = {n: k for n, k in ks.items() if "k_radiance_views" in n}
    assert len(views) == 9, sorted(views)
    assert len({n: k for n, k in ks.items() if "k_radiance_rays" in n}) == 9  # the memory-source forms are all still there
    lds = {n: k for n, k in views.items() if "Lb1E" in n}
    assert len(lds) == 1
    for n, k in lds.items():
        assert k[".vgpr_count"] <= 128 and k.get(".agpr_count", 0) == 0 and k.get(".vgpr_spill_count", 0) == 0, (n, k)
        assert k[".group_segment_fixed_size"] == 0 and k[".max_flat_workgroup_size"] == 1024, (n, k)
    sibling_spills = {"ILj127ELb0ELj3E": 2, "ILj127ELb0ELj15E": 3, "ILj127ELb0ELj19E": 3}
    for n, k in views.items():
        if n in lds:
            continue
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 168 and k[".group_segment_fixed_size"] == 0, (n, k)
        spill = next((v for tag, v in sibling_spills.items() if tag in n), 0)
        assert k.get(".vgpr_spill_count", 0) <= spill, (n, k.get(".vgpr_spill_count", 0), spill)
