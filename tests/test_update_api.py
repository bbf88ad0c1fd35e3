"""rt_scene_update_triangles, rt_scene_triangles_get, rt_scene_bvh_get: the exports and their bindings, rt_update_params'
layout, every refusal (each happens before a device is touched, with a message), rt_scene_triangles_get without a device,
the Python wrapper's buffer checks and the C++ facade.  Host-only.  (tests/test_scene.py's pinned scene hashes show that
moving conservative_box into refit.h changed no tree.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd import _lib
from another_raytracer_amd.scene import scene_dump
from another_raytracer_amd._lib import RT_GLOBAL_SCENE, RT_OUT_DEVICE, RT_PROFILE, lib, rt_update_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_OK, RT_E_INVALID, RT_E_DEVICE = 0, -1, -3
SYMBOLS = ("rt_scene_update_triangles", "rt_scene_triangles_get", "rt_scene_bvh_get")


def _tri(k):
    """Triangle k of the hand-built worlds: exact small doubles, all different."""
    return np.array([[k, 0.0, -k], [k + 1.0, 0.25 * k, -k], [k, 1.0, 0.5 - k]])


@pytest.fixture(scope="module")
def world():
    """Five triangles handed to a bvh_node in order 0..4, then a sphere and a sixth, loose triangle in the world list."""
    art.reset_scene_rng()
    grey = art.lambertian((0.5, 0.5, 0.5))
    w = art.hittable_list()
    w.add(art.bvh_node([art.triangle(*_tri(k), grey) for k in range(5)]))
    w.add(art.sphere((0, -100, 0), 50, grey))
    w.add(art.triangle(*_tri(5), grey))
    return art.compile_world(w, 0)


def _update(world, p="ok", first=0, n=None, scene=True, params=True, ms=False, **fields):
    count = lib.rt_scene_triangles_get(world, None, 0)
    if isinstance(p, str):
        p = np.arange(9.0 * count).reshape(count, 9)
    u = rt_update_params()
    for k, v in fields.items():
        setattr(u, k, v)
    t = ctypes.c_double(-1.0)
    return lib.rt_scene_update_triangles(world if scene else None, ctypes.byref(u) if params else None, None if p is None else ctypes.c_void_p(p.ctypes.data),
                                         first, (0 if p is None else len(p)) if n is None else n, ctypes.byref(t) if ms else None)


def _refused(world, **kw):
    return _update(world, **kw) == RT_E_INVALID and len(lib.rt_last_error()) > 0


def test_the_symbols_are_declared_exported_and_bound():
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "art.h")).read()
    for s in SYMBOLS:
        assert f" T {s}\n" in nm and s in _lib.SIGNATURES and f"{s}(rt_scene* scene" in header, s
    assert "(none: a scene is rebuilt every run)" in header and "typedef struct rt_update_params" in header
    for f in ("scene_triangles", "update_triangles", "scene_bvh"):
        assert callable(getattr(art, f)) and f in art.__all__
    assert lib.rt_abi_version() == 5  # the addition is additive


def test_rt_update_params_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    fields = [f for f, _ in rt_update_params._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "art.h"', "int main(void) {", 'printf("size %zu\\n", sizeof(rt_update_params));']
    lines += [f'printf("{f} %zu\\n", offsetof(rt_update_params, {f}));' for f in fields]
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(c["size"]) == ctypes.sizeof(rt_update_params) == 16
    for f in fields:
        assert int(c[f]) == getattr(rt_update_params, f).offset, f


def test_triangles_come_back_in_construction_order_without_a_device(world):
    assert lib.rt_scene_triangles_get(world, None, 0) == 6
    got = art.scene_triangles(world)
    assert got.shape == (6, 3, 3) and got.dtype == np.float64
    assert np.array_equal(got, np.stack([_tri(k) for k in range(6)]))  # the BVH's five in the order given, then the loose one
    small = np.zeros((5, 9))
    assert lib.rt_scene_triangles_get(world, ctypes.c_void_p(small.ctypes.data), 5) == RT_E_INVALID and b"6" in lib.rt_last_error()
    assert lib.rt_scene_triangles_get(None, None, 0) == RT_E_INVALID
    cow = art.scene_manager().build("cow")
    assert art.scene_triangles(cow).shape == (cow.info["triangles"], 3, 3) == (5804, 3, 3)
    assert art.scene_triangles(art.scene_manager().build("1")).shape == (0, 3, 3)


def test_null_arguments_and_ranges_are_refused(world):
    assert _refused(world, scene=False)
    assert _refused(world, params=False)
    assert _refused(world, p=None, n=1)                       # p NULL with n > 0
    assert _refused(world, first=-1, n=1)
    assert _refused(world, n=-1)
    assert _refused(world, first=1)                           # first + n = 7 > 6
    assert _refused(world, first=6, n=1)
    assert _refused(world, first=7, n=0)
    assert _refused(world, first=1 << 62, n=1 << 62)          # no overflow into range
    assert _refused(world, n=7)
    assert b"6 triangles" in lib.rt_last_error()


@pytest.mark.parametrize("flag", [RT_PROFILE, RT_GLOBAL_SCENE, 8, 16, 32, 64, 128, 256, 512, 1024, 1 << 30])
def test_other_flag_bits_are_refused(world, flag):
    assert _refused(world, flags=flag)
    assert _refused(world, flags=flag | RT_OUT_DEVICE)


def test_a_stream_without_rt_out_device_is_refused(world):
    assert _refused(world, stream=1234)
    assert b"RT_OUT_DEVICE" in lib.rt_last_error()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_in_a_host_buffer_is_refused(world, bad):
    for where in (0, 17, 53):
        p = np.arange(54.0).reshape(6, 9)
        p.flat[where] = bad
        assert _refused(world, p=p)
        assert f"triangle {where // 9}".encode() in lib.rt_last_error()
    p = np.arange(54.0).reshape(6, 9)
    p[0, 0] = bad  # a value outside the nine doubles per updated triangle is not looked at: the range check refuses this one
    assert _refused(world, p=p[1:3], first=5) and b"6 triangles" in lib.rt_last_error()


def test_degenerate_calls_are_ok_and_touch_no_device(world):
    # no device on a host-only machine: RT_OK shows the call returned before any device work
    assert _update(world, p=None, n=0) == RT_OK
    assert _update(world, n=0, first=6, ms=True) == RT_OK
    assert _update(world, n=0, flags=RT_OUT_DEVICE, stream=1234) == RT_OK
    spheres = art.scene_manager().build("c1").objects._native  # a scene without triangles accepts only n = 0
    assert _update(spheres, p=None, n=0) == RT_OK
    assert _refused(spheres, p=np.zeros((1, 9)), n=1)
    art.update_triangles(world, np.zeros((0, 3, 3)))
    assert scene_dump(art.scene_manager().build("c1"))  # a scene that was never updated still dumps


@pytest.mark.skipif(lib.rt_device_count() > 0, reason="checks the no-device failure path")
def test_valid_calls_without_a_device_fail_loudly(world):
    assert _update(world) == RT_E_DEVICE  # the arguments passed every check
    assert _update(world, p=np.ones((2, 9)), first=4, ms=True) == RT_E_DEVICE
    n = ctypes.c_int64()
    assert lib.rt_scene_bvh_get(world, None, 0, None, 0, ctypes.byref(n), None) == RT_E_DEVICE
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.update_triangles(world, art.scene_triangles(world))
    assert lib.rt_scene_bvh_get(None, None, 0, None, 0, None, None) == RT_E_INVALID


def test_python_wrapper_refuses_wrong_buffers_and_arguments(world):
    for bad in (np.zeros((6, 3, 3), np.float32), np.zeros((6, 3, 4)), np.zeros((6, 8)), np.zeros(54), np.zeros((6, 3, 6))[..., ::2],
                np.zeros((6, 3, 3, 1))):
        with pytest.raises(ValueError):
            art.update_triangles(world, bad)
    with pytest.raises(TypeError):
        art.update_triangles(world, [[0.0] * 9] * 6)
    with pytest.raises(ValueError):
        art.update_triangles(world, np.zeros((6, 3, 3)), stream=1234)  # a stream belongs to device tensors
    with pytest.raises(art.RTError, match="RT_E_INVALID"):
        art.update_triangles(world, np.zeros((6, 3, 3)), first=1)
    with pytest.raises(TypeError):
        art.update_triangles(art.hittable_list(), np.zeros((6, 3, 3)))  # not compiled
    with pytest.raises(TypeError):
        art.scene_triangles(None)
    with pytest.raises(TypeError):
        art.scene_bvh(art.hittable_list())
    import torch
    with pytest.raises(ValueError):
        art.update_triangles(world, torch.zeros((6, 3, 3), dtype=torch.float64))  # a tensor, but on the host
    assert art.deform.BVH_NODE.itemsize == 128 and art.deform.BVH_NODE.fields["child"][1] == 96


def test_the_cpp_facade_compiles(tmp_path):
    src = tmp_path / "u.cpp"
    src.write_text("""
#include "art_engine.hpp"
int main() {
    art::scene_manager sm("assets");
    art::scene world = sm.build("cow");
    std::vector<double> p = art::scene_triangles(world);
    for (double& x : p) x *= 1.5;
    double ms = 0;
    art::update_triangles(world, p.data(), 0, static_cast<std::int64_t>(p.size() / 9));
    art::update_triangles(world, p.data() + 9, 1, 2, 0, nullptr, &ms);
    return ms >= 0 ? 0 : 1;
}
""")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_refit_kernels_are_built_and_keep_their_values_in_registers():
    """k_update_tris and k_refit_level in the built code object: no spill and no scratch (a triangle's nine doubles, a
    slot's box and a child's six floats are the arrays that could end up there), no LDS."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(os.path.join(ROOT, "another_raytracer_amd", "libart.so"))
    for name in ("k_update_tris", "k_refit_level"):
        mine = [k for n, k in ks.items() if name in n]
        assert len(mine) == 1, (name, sorted(ks))
        k = mine[0]
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0 and k[".group_segment_fixed_size"] == 0, (name, k)
