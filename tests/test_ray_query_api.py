"""rt_query_rays: the struct layout, argument checks (every refusal happens before a device is touched), the Python
wrapper's buffer checks, the C++ facade and the new kernels' register budgets.  Host-only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import (RT_GLOBAL_SCENE, RT_HIT_DOUBLES, RT_OUT_DEVICE, RT_PROFILE, RT_Q_ANY_HIT, RT_Q_NO_MEDIA, lib,
                                        rt_query_params)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

RT_OK, RT_E_INVALID = 0, -1
N = 5


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def world():
    return art.scene_manager().build("c1")


def test_the_struct_and_constants_match_the_header(tmp_path):
    src = tmp_path / "q.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "art.h"', "int main(void) {",
             'printf("rt_query_params %zu\\n", sizeof(rt_query_params));']
    lines += [f'printf("rt_query_params.{f} %zu\\n", offsetof(rt_query_params, {f}));' for f, _ in rt_query_params._fields_]
    lines += [f'printf("{c} %d\\n", (int){c});' for c in ("RT_Q_ANY_HIT", "RT_Q_NO_MEDIA", "RT_HIT_DOUBLES", "RT_OUT_DEVICE", "RT_GLOBAL_SCENE")]
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "q"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(c["rt_query_params"]) == ctypes.sizeof(rt_query_params)
    for f, _ in rt_query_params._fields_:
        assert int(c[f"rt_query_params.{f}"]) == getattr(rt_query_params, f).offset, f
    assert (int(c["RT_Q_ANY_HIT"]), int(c["RT_Q_NO_MEDIA"]), int(c["RT_HIT_DOUBLES"])) == (RT_Q_ANY_HIT, RT_Q_NO_MEDIA, RT_HIT_DOUBLES) == (512, 1024, 12)
    assert (int(c["RT_OUT_DEVICE"]), int(c["RT_GLOBAL_SCENE"])) == (RT_OUT_DEVICE, RT_GLOBAL_SCENE)
    # a zero-initialised struct asks for the closest hit on host buffers on the scene's stream
    z = rt_query_params()
    assert z.flags == 0 and z.reserved == 0 and z.stream is None


def _call(world, flags=0, n=N, scene=True, params=True, hits=True, occluded=False, rays=True):
    r = np.zeros((max(n, 1), 7))
    h = np.zeros((max(n, 1), RT_HIT_DOUBLES))
    o = np.zeros(max(n, 1), np.uint8)
    q = rt_query_params(flags=flags)
    return lib.rt_query_rays(world.objects._native if scene else None, ctypes.byref(q) if params else None, _ptr(r) if rays else None, None, n,
                             _ptr(h) if hits else None, _ptr(o) if occluded else None)


def _refused(world, **kw):
    return _call(world, **kw) == RT_E_INVALID and len(lib.rt_last_error()) > 0


def test_null_scene_and_params_are_refused(world):
    assert _refused(world, scene=False)
    assert _refused(world, params=False)
    assert _refused(world, rays=False)


@pytest.mark.parametrize("n", [-1, (1 << 30) + 1, 1 << 40])
def test_ray_counts_outside_the_range_are_refused(world, n):
    q = rt_query_params()
    one = np.zeros(RT_HIT_DOUBLES)
    assert lib.rt_query_rays(world.objects._native, ctypes.byref(q), _ptr(one), None, n, _ptr(one), None) == RT_E_INVALID
    assert b"n must be" in lib.rt_last_error()


@pytest.mark.parametrize("flag", [RT_PROFILE, 8, 16, 32, 64, 128, 256, 2048, 1 << 30])
def test_unknown_flag_bits_are_refused(world, flag):
    assert _refused(world, flags=flag)
    assert _refused(world, flags=flag | RT_Q_ANY_HIT, hits=False, occluded=True)


def test_the_output_pointers_must_match_the_mode(world):
    assert _refused(world, hits=True, occluded=True)                        # both
    assert _refused(world, hits=False, occluded=False)                      # neither
    assert _refused(world, flags=RT_Q_ANY_HIT, hits=True, occluded=True)
    assert _refused(world, flags=RT_Q_ANY_HIT, hits=False, occluded=False)
    assert _refused(world, flags=RT_Q_ANY_HIT, hits=True, occluded=False)   # the any-hit flag with the closest-mode buffer
    assert _refused(world, flags=0, hits=False, occluded=True)              # the occlusion buffer without the flag
    assert _refused(world, flags=RT_Q_NO_MEDIA, hits=False, occluded=True)


@pytest.mark.parametrize("flags,any_hit", [(0, False), (RT_Q_NO_MEDIA | RT_GLOBAL_SCENE, False), (RT_Q_ANY_HIT, True),
                                           (RT_Q_ANY_HIT | RT_Q_NO_MEDIA | RT_OUT_DEVICE, True), (RT_OUT_DEVICE, False)])
def test_zero_rays_is_ok_and_touches_no_device(world, flags, any_hit):
    # no device on a host-only machine: RT_OK shows the call returned before any device work
    assert _call(world, flags=flags, n=0, hits=not any_hit, occluded=any_hit) == RT_OK
    assert _call(world, flags=flags, n=0, hits=not any_hit, occluded=any_hit, rays=False) == RT_OK


@pytest.mark.skipif(lib.rt_device_count() > 0, reason="checks the no-device failure path")
def test_a_valid_call_without_a_device_fails_loudly(world):
    assert _call(world) == -3  # RT_E_DEVICE: the arguments passed every check
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.query_rays(world.objects, np.zeros((N, 7)))


def test_python_wrapper_refuses_wrong_dtypes_shapes_and_strides(world):
    rays = np.zeros((N, 7))
    for bad in (rays.astype(np.float32), np.zeros((N, 6)), np.zeros(7 * N), np.zeros((N, 14))[:, ::2], np.zeros((7, N)).T, np.zeros((2, N, 7))):
        with pytest.raises(ValueError):
            art.query_rays(world.objects, bad)
    with pytest.raises(TypeError):
        art.query_rays(world.objects, rays.tolist())
    for bad in (np.zeros(N, np.float32), np.zeros(N + 1), np.zeros((N, 1)), np.zeros(2 * N)[::2]):
        with pytest.raises(ValueError):
            art.query_rays(world.objects, rays, t_max=bad)
    with pytest.raises(TypeError):
        art.query_rays(world.objects, rays, t_max=[1.0] * N)
    for bad in (np.zeros((N, 12), np.float32), np.zeros((N, 10)), np.zeros((N + 1, 12)), np.zeros((N, 24))[:, ::2], np.zeros(N, np.uint8)):
        with pytest.raises(ValueError):
            art.query_rays(world.objects, rays, out=bad)
    for bad in (np.zeros(N, np.int32), np.zeros(N + 1, np.uint8), np.zeros(2 * N, np.uint8)[::2], np.zeros((N, 12))):
        with pytest.raises(ValueError):
            art.query_rays(world.objects, rays, any_hit=True, out=bad)
    with pytest.raises(ValueError):
        art.query_rays(world.objects, rays, stream=1234)  # a stream belongs to device tensors
    with pytest.raises(TypeError):
        art.query_rays(art.hittable_list(), rays)          # not compiled
    with pytest.raises(TypeError):
        art.query_rays(None, rays)


def test_python_wrapper_refuses_host_tensors_and_mixed_buffers(world):
    import torch
    rays = np.zeros((N, 7))
    with pytest.raises(ValueError):
        art.query_rays(world.objects, torch.zeros((N, 7), dtype=torch.float64))   # a tensor, but on the host
    with pytest.raises(ValueError):
        art.query_rays(world.objects, rays, t_max=torch.zeros(N, dtype=torch.float64))
    with pytest.raises(ValueError):
        art.query_rays(world.objects, rays, out=torch.zeros((N, 12), dtype=torch.float64))


def test_hit_records_name_their_columns():
    rec = np.arange(2 * RT_HIT_DOUBLES, dtype=np.float64).reshape(2, RT_HIT_DOUBLES)
    h = art.HitRecords(rec)
    assert len(h) == 2 and h.t.tolist() == [0, 12] and h.normal.tolist() == [[1, 2, 3], [13, 14, 15]]
    assert h.point[1].tolist() == [16, 17, 18] and (h.u[0], h.v[0], h.front_face[0], h.prim[0], h.mat[0]) == (7, 8, 9, 10, 11)
    assert np.array_equal(np.asarray(h), rec)
    with pytest.raises(AttributeError):
        h.albedo


def test_the_new_kernels_are_in_the_library_and_spill_nothing():
    ks = kernel_resources.kernels(os.path.join(ROOT, "another_raytracer_amd", "libart.so"))
    query = {n: k for n, k in ks.items() if "k_query_rays" in n}
    occlude = {n: k for n, k in ks.items() if "k_occlude_rays" in n}
    # the LDS image and the three HBM-scene feature sets; the any-hit kernels in both child orders (option query.any_sorted)
    assert len(query) == 4 and len(occlude) == 8, (sorted(query), sorted(occlude))
    for n, k in {**query, **occlude}.items():
        assert k.get(".vgpr_spill_count", 0) == 0, (n, k)
        # the LDS-image variants run one 1024-lane block per CU: 16 waves, 4 per SIMD, 512 / 4 = 128 VGPRs each
        if "Lb1E" in n:
            assert k[".vgpr_count"] <= 128 and k[".group_segment_fixed_size"] == 0, (n, k)
    assert sum("Lb1E" in n for n in query) == 1 and sum("Lb1E" in n for n in occlude) == 2


def test_the_option_that_picks_the_any_hit_child_order():
    default = art.get_option("query.any_sorted")
    assert default in (0, 1)
    try:
        art.set_option("query.any_sorted", 1 - default)
        assert art.get_option("query.any_sorted") == 1 - default
        with pytest.raises(art.RTError):
            art.set_option("query.any_sorted", 2)
    finally:
        art.set_option("query.any_sorted", default)


def test_the_cpp_facade_compiles(tmp_path):
    src = tmp_path / "q.cpp"
    src.write_text("""
#include "art_engine.hpp"
int main() {
    art::scene_manager sm("assets");
    art::scene world = sm.build("6");
    std::vector<double> rays(7 * 3, 0.0), t_max(3, 10.0), hits(3 * RT_HIT_DOUBLES);
    std::vector<std::uint8_t> occ(3);
    art::query_rays(world, rays.data(), nullptr, 3, hits.data());
    art::query_rays(world, rays.data(), t_max.data(), 3, hits.data(), RT_Q_NO_MEDIA | RT_GLOBAL_SCENE);
    art::occluded_rays(world, rays.data(), t_max.data(), 3, occ.data());
    return occ[0] <= 1 ? 0 : 1;
}
""")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
