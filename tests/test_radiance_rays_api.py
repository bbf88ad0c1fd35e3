"""rt_radiance_rays / rt_camera_rays: the struct layout, argument checks (every refusal happens before a device is touched),
the Python wrappers' buffer checks, the C++ facade and the new kernels' register budgets.  Host-only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import RT_GLOBAL_SCENE, RT_OUT_DEVICE, RT_PROFILE, lib, rt_camera, rt_params, rt_radiance_params, rt_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

RT_OK, RT_E_INVALID, RT_E_DEVICE = 0, -1, -3
N = 5


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def world():
    return art.scene_manager().build("c1")


def test_the_struct_matches_the_header(tmp_path):
    src = tmp_path / "q.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "art.h"', "int main(void) {",
             'printf("rt_radiance_params %zu\\n", sizeof(rt_radiance_params));']
    lines += [f'printf("rt_radiance_params.{f} %zu\\n", offsetof(rt_radiance_params, {f}));' for f, _ in rt_radiance_params._fields_]
    lines += [f'printf("{c} %d\\n", (int){c});' for c in ("RT_OUT_DEVICE", "RT_GLOBAL_SCENE", "RT_ABI_VERSION")]
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "q"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(c["rt_radiance_params"]) == ctypes.sizeof(rt_radiance_params) == 64
    for f, _ in rt_radiance_params._fields_:
        assert int(c[f"rt_radiance_params.{f}"]) == getattr(rt_radiance_params, f).offset, f
    assert (int(c["RT_OUT_DEVICE"]), int(c["RT_GLOBAL_SCENE"])) == (RT_OUT_DEVICE, RT_GLOBAL_SCENE)
    assert int(c["RT_ABI_VERSION"]) == 5  # the additions are additive
    # a zero-initialised struct plus max_depth asks for one sample per ray on host buffers with seed 0
    z = rt_radiance_params()
    assert (z.flags, z.spp, z.sample_base, z.seed, z.id_base, z.stream) == (0, 0, 0, 0, 0, None)
    assert "rt_radiance_rays" in art._lib.SIGNATURES and "rt_camera_rays" in art._lib.SIGNATURES


def _call(world, n=N, scene=True, params=True, rays=True, radiance=True, rng=False, stats=False, **fields):
    r = np.zeros((max(n, 1), 7))
    out = np.zeros((max(n, 1), 3))
    q = rt_radiance_params(max_depth=50)
    for k, v in fields.items():
        setattr(q, k, v)
    states = np.zeros(max(n, 1) * max(q.spp, 1), np.uint64) if rng else None
    st = rt_stats()
    return lib.rt_radiance_rays(world.objects._native if scene else None, ctypes.byref(q) if params else None, _ptr(r) if rays else None,
                                _ptr(states) if rng else None, n, _ptr(out) if radiance else None, ctypes.byref(st) if stats else None)


def _refused(world, **kw):
    return _call(world, **kw) == RT_E_INVALID and len(lib.rt_last_error()) > 0


def test_null_arguments_are_refused(world):
    assert _refused(world, scene=False)
    assert _refused(world, params=False)
    assert _refused(world, rays=False)
    assert _refused(world, radiance=False)


@pytest.mark.parametrize("n", [-1, (1 << 30) + 1, 1 << 40])
def test_ray_counts_outside_the_range_are_refused(world, n):
    q = rt_radiance_params(max_depth=50)
    one = np.zeros(7)
    assert lib.rt_radiance_rays(world.objects._native, ctypes.byref(q), _ptr(one), None, n, _ptr(one), None) == RT_E_INVALID
    assert b"n must be" in lib.rt_last_error()


def test_more_paths_than_a_call_holds_are_refused_with_the_limit_named(world):
    q = rt_radiance_params(max_depth=50, spp=3)
    one = np.zeros(7)
    # 2^30 rays x 3 samples > 2^31 paths; 2^30 x 2 is exactly the limit and passes the check (it then needs a device)
    assert lib.rt_radiance_rays(world.objects._native, ctypes.byref(q), _ptr(one), None, 1 << 30, _ptr(one), None) == RT_E_INVALID
    assert b"kMaxPassSlots" in lib.rt_last_error() and b"2^31" in lib.rt_last_error()
    q.spp = 1 << 30
    assert lib.rt_radiance_rays(world.objects._native, ctypes.byref(q), _ptr(one), None, 3, _ptr(one), None) == RT_E_INVALID


@pytest.mark.parametrize("flag", [RT_PROFILE, 8, 16, 32, 64, 128, 256, 512, 1024, 1 << 30])
def test_unknown_flag_bits_are_refused(world, flag):
    assert _refused(world, flags=flag)
    assert _refused(world, flags=flag | RT_OUT_DEVICE)


def test_parameters_outside_their_range_are_refused(world):
    assert _refused(world, max_depth=0)
    assert _refused(world, max_depth=-1)
    assert _refused(world, spp=-1)
    assert _refused(world, stream=1234)                      # a stream without RT_OUT_DEVICE
    assert _refused(world, id_base=(1 << 32) - N + 1)        # id_base + n > 2^32
    assert _refused(world, id_base=1 << 63)
    assert _refused(world, id_base=(1 << 64) - 1)            # must not wrap


@pytest.mark.parametrize("fields", [{}, {"flags": RT_OUT_DEVICE}, {"flags": RT_GLOBAL_SCENE, "spp": 8}, {"flags": RT_OUT_DEVICE, "stream": 1234}])
def test_zero_rays_is_ok_and_touches_no_device(world, fields):
    # no device on a host-only machine: RT_OK shows the call returned before any device work
    assert _call(world, n=0, **fields) == RT_OK
    assert _call(world, n=0, rays=False, radiance=False, stats=True, **fields) == RT_OK


@pytest.mark.skipif(lib.rt_device_count() > 0, reason="checks the no-device failure path")
def test_a_valid_call_without_a_device_fails_loudly(world):
    assert _call(world) == RT_E_DEVICE  # the arguments passed every check
    assert _call(world, spp=0) == RT_E_DEVICE                               # 0 samples is taken as 1
    assert _call(world, id_base=(1 << 32) - N, spp=4) == RT_E_DEVICE        # the last valid stream id
    assert _call(world, id_base=(1 << 63), rng=True) == RT_E_DEVICE         # id_base is ignored when states are given
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.radiance_rays(world, np.zeros((N, 7)))
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, 16 / 9, world.aperture, 10.0)
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.camera_rays(cam, 16, 9, 2)


def _camera_call(width=16, height=9, spp=2, flags=0, stream=None, cam=True, rays=True, device=0, band=(9, 1, 0)):
    c = rt_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 16 / 9, 0.1, 5.0, 0.0, 1.0)
    p = rt_params(width=width, height=height, spp=spp, flags=flags, stream=stream, band_rows=band[0], band_count=band[1], band_index=band[2])
    out = np.zeros((max(width * height * spp, 1), 7))
    return lib.rt_camera_rays(ctypes.byref(c) if cam else None, ctypes.byref(p), 0, device, _ptr(out) if rays else None, None)


def test_camera_rays_refuses_bad_arguments_before_any_device_work():
    for kw in ({"cam": False}, {"rays": False}, {"width": 1}, {"height": 1}, {"spp": 0}, {"flags": RT_GLOBAL_SCENE}, {"flags": RT_PROFILE},
               {"stream": 1234}, {"device": -1}, {"band": (0, 1, 0)}, {"band": (4, 2, 2)}):
        assert _camera_call(**kw) == RT_E_INVALID and len(lib.rt_last_error()) > 0, kw
    c = rt_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 5.0, 0.0, 1.0)
    assert lib.rt_camera_rays(ctypes.byref(c), None, 0, 0, _ptr(np.zeros(7)), None) == RT_E_INVALID
    # 4096 x 4096 pixels x 256 samples = 2^32 ray slots: more than one call holds
    p = rt_params(width=4096, height=4096, spp=256, band_rows=4096, band_count=1)
    assert lib.rt_camera_rays(ctypes.byref(c), ctypes.byref(p), 0, 0, _ptr(np.zeros(7)), None) == RT_E_INVALID
    assert b"kMaxPassSlots" in lib.rt_last_error()


def test_python_wrapper_refuses_wrong_dtypes_shapes_and_strides(world):
    rays = np.zeros((N, 7))
    for bad in (rays.astype(np.float32), np.zeros((N, 6)), np.zeros(7 * N), np.zeros((N, 14))[:, ::2], np.zeros((7, N)).T, np.zeros((2, N, 7))):
        with pytest.raises(ValueError):
            art.radiance_rays(world, bad)
    with pytest.raises(TypeError):
        art.radiance_rays(world, rays.tolist())
    # rng: n * spp uint64 states
    for bad in (np.zeros(N, np.int64), np.zeros(N, np.float64), np.zeros(N + 1, np.uint64), np.zeros((N, 1), np.uint64), np.zeros(2 * N, np.uint64)[::2]):
        with pytest.raises(ValueError):
            art.radiance_rays(world, rays, rng=bad)
    with pytest.raises(ValueError):
        art.radiance_rays(world, rays, spp=3, rng=np.zeros(N, np.uint64))      # the wrong length for 3 samples per ray
    with pytest.raises(ValueError):
        art.radiance_rays(world, rays, spp=2, rng=np.zeros(3 * N, np.uint64))
    with pytest.raises(TypeError):
        art.radiance_rays(world, rays, rng=[0] * N)
    for bad in (np.zeros((N, 3), np.float32), np.zeros((N, 4)), np.zeros((N + 1, 3)), np.zeros((N, 6))[:, ::2], np.zeros(3 * N)):
        with pytest.raises(ValueError):
            art.radiance_rays(world, rays, out=bad)
    with pytest.raises(ValueError):
        art.radiance_rays(world, rays, spp=0)
    with pytest.raises(ValueError):
        art.radiance_rays(world, rays, stream=1234)  # a stream belongs to device tensors
    with pytest.raises(TypeError):
        art.radiance_rays(art.hittable_list(), rays)  # not compiled
    with pytest.raises(TypeError):
        art.radiance_rays(None, rays)
    with pytest.raises(TypeError):
        art.camera_rays(None, 16, 9, 1)
    cam = art.camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 16 / 9, 0.0, 5.0)
    with pytest.raises(ValueError):
        art.camera_rays(cam, 16, 9, 0)
    with pytest.raises(ValueError):
        art.camera_rays(cam, 16, 9, 1, stream=1234)
    with pytest.raises(ValueError):
        art.camera_rays(cam, 16, 9, 1, device="cpu")


def test_python_wrapper_refuses_host_tensors_and_mixed_buffers(world):
    import torch
    rays = np.zeros((N, 7))
    with pytest.raises(ValueError):
        art.radiance_rays(world, torch.zeros((N, 7), dtype=torch.float64))   # a tensor, but on the host
    with pytest.raises(ValueError):
        art.radiance_rays(world, rays, rng=torch.zeros(N, dtype=torch.int64))
    with pytest.raises(ValueError):
        art.radiance_rays(world, rays, out=torch.zeros((N, 3), dtype=torch.float64))


def test_the_cpp_facade_compiles(tmp_path):
    src = tmp_path / "q.cpp"
    src.write_text("""
#include "art_engine.hpp"
int main() {
    art::scene_manager sm("assets");
    art::scene world = sm.build("6");
    art::camera cam(world.lookfrom, world.lookat, art::vec3{{0, 1, 0}}, world.vfov, 16.0 / 9.0, world.aperture, 10.0, 0.0, 1.0);
    const int W = 16, H = 9, k = 2;
    std::vector<double> rays(7 * W * H * k), radiance(3 * W * H * k);
    std::vector<std::uint64_t> rng(W * H * k);
    art::camera_rays(cam, W, H, k, rays.data(), rng.data(), 3);
    art::camera_rays(cam, W, H, k, rays.data(), nullptr);
    art::radiance_options o;
    o.max_depth = 20;
    o.background = world.background;
    rt_stats st{};
    art::radiance_rays(world, rays.data(), W * H * k, radiance.data(), o, rng.data(), &st);
    o.spp = 4;
    o.seed = 9;
    o.id_base = 100;
    art::radiance_rays(world, rays.data(), W * H * k, radiance.data(), o);
    return st.segments >= st.primary ? 0 : 1;
}
""")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_new_kernels_are_in_the_library_and_meet_their_register_budgets():
    ks = kernel_resources.kernels(os.path.join(ROOT, "another_raytracer_amd", "libart.so"))
    rad = {n: k for n, k in ks.items() if "k_radiance_rays" in n}
    # the LDS scene image with solid / checker textures; the three HBM-scene feature sets with solid / checker or all
    # textures, the two with triangles also with barycentric images
    assert len(rad) == 9, sorted(rad)
    lds = {n: k for n, k in rad.items() if "Lb1E" in n}
    assert len(lds) == 1
    for n, k in lds.items():
        # one 1024-lane block per CU: 16 waves, 4 per SIMD, 512 / 4 = 128 VGPRs each; the image starts at LDS address 0
        assert k[".vgpr_count"] <= 128 and k.get(".agpr_count", 0) == 0 and k.get(".vgpr_spill_count", 0) == 0, (n, k)
        assert k[".group_segment_fixed_size"] == 0 and k[".max_flat_workgroup_size"] == 1024, (n, k)
    # the HBM-scene forms keep three waves per SIMD (168 VGPRs).  All spill nothing but the three F_ALL forms (every
    # primitive type, transforms, medium boundaries): k_radiance_rays<127, false, 3 / 15 / 19> park 2 / 3 / 3 VGPRs
    allowed = {"ILj127ELb0ELj3E": 2, "ILj127ELb0ELj15E": 3, "ILj127ELb0ELj19E": 3}
    for n, k in rad.items():
        if n in lds:
            continue
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 168 and k[".group_segment_fixed_size"] == 0, (n, k)
        spill = next((v for tag, v in allowed.items() if tag in n), 0)
        assert k.get(".vgpr_spill_count", 0) <= spill, (n, k)
    for name in ("k_radiance_sum", "k_camera_rays"):
        found = [k for n, k in ks.items() if name in n]
        assert len(found) == 1 and found[0].get(".vgpr_spill_count", 0) == 0 and found[0].get(".private_segment_fixed_size", 0) == 0, name
