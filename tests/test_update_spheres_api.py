"""rt_scene_update_spheres, rt_scene_spheres_get, rt_scene_lds_image_get: the exports and their bindings, every refusal
(each happens before a device is touched, with a message), rt_scene_spheres_get without a device, the Python wrapper's
buffer checks and the C++ facade.  Host-only.  (tests/test_scene.py's pinned scene hashes and the parity tests show that
moving the image builder's arithmetic into lds_image.h changed no byte.)"""
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
SYMBOLS = ("rt_scene_update_spheres", "rt_scene_spheres_get", "rt_scene_lds_image_get")


def _sph(k):
    """Sphere k of the hand-built world: exact small doubles, all different."""
    return np.array([k, 0.25 * k, -2.0 * k, 0.5 + 0.125 * k])


@pytest.fixture(scope="module")
def world():
    """Five spheres handed to a bvh_node in order 0..4 (number 2 a moving_sphere), a triangle, then two loose spheres and
    a constant_medium with a sphere boundary in the world list: 8 spheres."""
    art.reset_scene_rng()
    grey = art.lambertian((0.5, 0.5, 0.5))
    w = art.hittable_list()
    inner = []
    for k in range(5):
        s = _sph(k)
        inner.append(art.moving_sphere(s[:3], s[:3] + (0.0, 0.5, 0.0), 0.0, 1.0, s[3], grey) if k == 2 else art.sphere(s[:3], s[3], grey))
    w.add(art.bvh_node(inner))
    w.add(art.triangle((0, 0, 5), (1, 0, 5), (0, 1, 5), grey))
    w.add(art.sphere(_sph(5)[:3], _sph(5)[3], grey))
    w.add(art.constant_medium(art.sphere(_sph(6)[:3], _sph(6)[3], grey), 0.01, (1, 1, 1)))
    w.add(art.sphere(_sph(7)[:3], _sph(7)[3], grey))
    return art.compile_world(w, 0)


N = 8


def _update(world, s="ok", first=0, n=None, scene=True, params=True, ms=False, **fields):
    count = lib.rt_scene_spheres_get(world, None, 0)
    if isinstance(s, str):
        s = np.arange(1.0, 4.0 * count + 1.0).reshape(count, 4)
    u = rt_update_params()
    for k, v in fields.items():
        setattr(u, k, v)
    t = ctypes.c_double(-1.0)
    return lib.rt_scene_update_spheres(world if scene else None, ctypes.byref(u) if params else None, None if s is None else ctypes.c_void_p(s.ctypes.data),
                                       first, (0 if s is None else len(s)) if n is None else n, ctypes.byref(t) if ms else None)


def _refused(world, **kw):
    return _update(world, **kw) == RT_E_INVALID and len(lib.rt_last_error()) > 0


def test_the_symbols_are_declared_exported_and_bound():
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "art.h")).read()
    for s in SYMBOLS:
        assert f" T {s}\n" in nm and s in _lib.SIGNATURES and f"{s}(rt_scene* scene" in header, s
    for f in ("scene_spheres", "update_spheres", "scene_lds_image"):
        assert callable(getattr(art, f)) and f in art.__all__
    assert lib.rt_abi_version() == 5  # the addition is additive


def test_spheres_come_back_in_compiled_order_without_a_device(world):
    assert lib.rt_scene_spheres_get(world, None, 0) == N
    got = art.scene_spheres(world)
    assert got.shape == (N, 4) and got.dtype == np.float64
    # the BVH's five in the order given (the moving one by its center0), then the world list's: loose, boundary, loose
    assert np.array_equal(got, np.stack([_sph(k) for k in range(N)]))
    small = np.zeros((N - 1, 4))
    assert lib.rt_scene_spheres_get(world, ctypes.c_void_p(small.ctypes.data), N - 1) == RT_E_INVALID and str(N).encode() in lib.rt_last_error()
    assert lib.rt_scene_spheres_get(None, None, 0) == RT_E_INVALID
    one = art.scene_manager().build("1")
    s = art.scene_spheres(one)
    assert s.shape == (one.info["spheres"], 4) and (s[:, 3] > 0).all() and np.isfinite(s).all()
    assert (s[0] == (0.0, -1000.0, 0.0, 1000.0)).all()  # the ground comes first (scene_manager.cpp random_scene)
    assert art.scene_spheres(art.scene_manager().build("cow")).shape[1] == 4


def test_null_arguments_and_ranges_are_refused(world):
    assert _refused(world, scene=False)
    assert _refused(world, params=False)
    assert _refused(world, s=None, n=1)                       # s NULL with n > 0
    assert _refused(world, first=-1, n=1)
    assert _refused(world, n=-1)
    assert _refused(world, first=1)                           # first + n = 9 > 8
    assert _refused(world, first=N, n=1)
    assert _refused(world, first=N + 1, n=0)
    assert _refused(world, first=1 << 62, n=1 << 62)          # no overflow into range
    assert _refused(world, n=N + 1)
    assert b"8 spheres" in lib.rt_last_error()


@pytest.mark.parametrize("flag", [RT_PROFILE, RT_GLOBAL_SCENE, 8, 16, 32, 64, 128, 256, 512, 1024, 1 << 30])
def test_other_flag_bits_are_refused(world, flag):
    assert _refused(world, flags=flag)
    assert _refused(world, flags=flag | RT_OUT_DEVICE)


def test_a_stream_without_rt_out_device_is_refused(world):
    assert _refused(world, stream=1234)
    assert b"RT_OUT_DEVICE" in lib.rt_last_error()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_in_a_host_buffer_is_refused(world, bad):
    for where in (0, 7, 4 * N - 1):
        s = np.arange(1.0, 4.0 * N + 1.0).reshape(N, 4)
        s.flat[where] = bad
        assert _refused(world, s=s)
        assert f"sphere {where // 4}".encode() in lib.rt_last_error()
    s = np.arange(1.0, 4.0 * N + 1.0).reshape(N, 4)
    s[0, 0] = bad  # a value outside the four doubles per updated sphere is not looked at: the range check refuses this one
    assert _refused(world, s=s[1:3], first=N - 1) and b"8 spheres" in lib.rt_last_error()


@pytest.mark.parametrize("bad", [0.0, -0.0, -1.0, -1e-300])
def test_a_radius_that_is_not_positive_in_a_host_buffer_is_refused(world, bad):
    for k in (0, 3, N - 1):
        s = np.arange(1.0, 4.0 * N + 1.0).reshape(N, 4)
        s[k, 3] = bad
        assert _refused(world, s=s)
        assert f"radius of sphere {k} ".encode() in lib.rt_last_error()
    s = np.full((N, 4), -5.0)  # negative centres are fine
    s[:, 3] = 1e-300
    assert _update(world, s=s, n=0) == RT_OK
    s[2, 3] = bad
    assert _refused(world, s=s[2:3], first=4) and b"sphere 4 " in lib.rt_last_error()  # numbered as in the scene


def test_degenerate_calls_are_ok_and_touch_no_device(world):
    # no device on a host-only machine: RT_OK shows the call returned before any device work
    assert _update(world, s=None, n=0) == RT_OK
    assert _update(world, n=0, first=N, ms=True) == RT_OK
    assert _update(world, n=0, flags=RT_OUT_DEVICE, stream=1234) == RT_OK
    art.reset_scene_rng()
    w = art.hittable_list()
    w.add(art.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), art.lambertian((0.5, 0.5, 0.5))))
    none = art.compile_world(w, 0)  # a scene without spheres accepts only n = 0
    assert lib.rt_scene_spheres_get(none, None, 0) == 0 and art.scene_spheres(none).shape == (0, 4)
    assert _update(none, s=None, n=0) == RT_OK
    assert _refused(none, s=np.ones((1, 4)), n=1)
    art.update_spheres(world, np.zeros((0, 4)))
    assert scene_dump(art.scene_manager().build("c1"))  # a scene that was never updated still dumps


@pytest.mark.skipif(lib.rt_device_count() > 0, reason="checks the no-device failure path")
def test_valid_calls_without_a_device_fail_loudly(world):
    assert _update(world) == RT_E_DEVICE  # the arguments passed every check
    assert _update(world, s=np.ones((2, 4)), first=4, ms=True) == RT_E_DEVICE
    assert lib.rt_scene_lds_image_get(world, 0, None, 0) == RT_E_DEVICE
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.update_spheres(world, art.scene_spheres(world))
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.scene_lds_image(world)


def test_lds_image_get_refuses_bad_arguments_before_a_device(world):
    assert lib.rt_scene_lds_image_get(None, 0, None, 0) == RT_E_INVALID
    assert lib.rt_scene_lds_image_get(world, 2, None, 0) == RT_E_INVALID and b"rebuilt" in lib.rt_last_error()
    assert lib.rt_scene_lds_image_get(world, -1, None, 0) == RT_E_INVALID


def test_python_wrapper_refuses_wrong_buffers_and_arguments(world):
    for bad in (np.zeros((N, 4), np.float32), np.zeros((N, 3)), np.zeros((N, 5)), np.zeros(4 * N), np.zeros((N, 8))[:, ::2], np.zeros((N, 4, 1))):
        with pytest.raises(ValueError):
            art.update_spheres(world, bad)
    with pytest.raises(TypeError):
        art.update_spheres(world, [[0.0, 0.0, 0.0, 1.0]] * N)
    with pytest.raises(ValueError):
        art.update_spheres(world, np.ones((N, 4)), stream=1234)  # a stream belongs to device tensors
    with pytest.raises(art.RTError, match="RT_E_INVALID"):
        art.update_spheres(world, np.ones((N, 4)), first=1)
    with pytest.raises(art.RTError, match="RT_E_INVALID"):
        art.update_spheres(world, np.zeros((N, 4)))  # radius 0
    with pytest.raises(TypeError):
        art.update_spheres(art.hittable_list(), np.ones((N, 4)))  # not compiled
    with pytest.raises(TypeError):
        art.scene_spheres(None)
    with pytest.raises(TypeError):
        art.scene_lds_image(art.hittable_list())
    import torch
    with pytest.raises(ValueError):
        art.update_spheres(world, torch.ones((N, 4), dtype=torch.float64))  # a tensor, but on the host


def test_the_cpp_facade_compiles(tmp_path):
    src = tmp_path / "u.cpp"
    src.write_text("""
#include "art_engine.hpp"
int main() {
    art::scene_manager sm("assets");
    art::scene world = sm.build("1");
    std::vector<double> s = art::scene_spheres(world);
    for (std::size_t k = 0; k < s.size(); k += 4) s[k + 1] += 0.25;
    double ms = 0;
    art::update_spheres(world, s.data(), 0, static_cast<std::int64_t>(s.size() / 4));
    art::update_spheres(world, s.data() + 4, 1, 2, 0, nullptr, &ms);
    return ms >= 0 ? 0 : 1;
}
""")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_sphere_update_kernels_are_built_and_keep_their_values_in_registers():
    """k_update_spheres and k_image_nodes in the built code object: no spill and no scratch (a sphere record, a slot's box
    and a node's planes are the arrays that could end up there), no LDS."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(os.path.join(ROOT, "another_raytracer_amd", "libart.so"))
    for name in ("k_update_spheres", "k_image_nodes"):
        mine = [k for n, k in ks.items() if name in n]
        assert len(mine) == 1, (name, sorted(ks))
        k = mine[0]
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0 and k[".group_segment_fixed_size"] == 0, (name, k)
