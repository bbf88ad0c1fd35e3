"""rt_render_guides / rt_denoise / rt_render_denoised argument checks and the new kernels' register budgets: host-only
(every refusal happens before a device is touched)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import (RT_ADAPTIVE, RT_DN_NO_DEMODULATE, RT_GUIDE_DOUBLES, RT_OUT_DEVICE, RT_PARALLEL_IMAGES, RT_PROFILE,
                                        RT_SPLIT_SHADE, lib, rt_denoise_params, rt_stats)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

RT_E_INVALID = -1
W, H = 8, 6


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def eng():
    world = art.scene_manager().build("c1")
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    e = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=4)
    e.set_scene(world.objects, world.background)
    return e


def _denoise(p, a=True, b=True, g=True, out=True, spp=2):
    acc = np.zeros((H, W, 3))
    guides = np.zeros((H, W, RT_GUIDE_DOUBLES))
    res = np.zeros((H, W, 3))
    return lib.rt_denoise(0, ctypes.byref(p) if p is not None else None, _ptr(acc) if a else None, _ptr(acc) if b else None, spp,
                          _ptr(guides) if g else None, _ptr(res) if out else None, None, None)


def _dn(**kw):
    p = rt_denoise_params()
    p.width, p.height = W, H
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_the_struct_and_constants_match_the_header(tmp_path):
    import subprocess
    src = tmp_path / "dn.c"
    fields = [f for f, _ in rt_denoise_params._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "art.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rt_denoise_params));', 'printf("guide %d\\n", RT_GUIDE_DOUBLES);',
             'printf("nodemod %d\\n", RT_DN_NO_DEMODULATE);']
    lines += [f'printf("{f} %zu\\n", offsetof(rt_denoise_params, {f}));' for f in fields]
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "dn"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(c["size"]) == ctypes.sizeof(rt_denoise_params)
    assert int(c["guide"]) == RT_GUIDE_DOUBLES and int(c["nodemod"]) == RT_DN_NO_DEMODULATE
    for f in fields:
        assert int(c[f]) == getattr(rt_denoise_params, f).offset, f


@pytest.mark.parametrize("case", ["params", "accum_a", "accum_b", "guides", "out_color"])
def test_denoise_refuses_null_buffers(case):
    args = {"a": case != "accum_a", "b": case != "accum_b", "g": case != "guides", "out": case != "out_color"}
    assert _denoise(None if case == "params" else _dn(), **args) == RT_E_INVALID
    assert "NULL" in lib.rt_last_error().decode()


@pytest.mark.parametrize("bad", [{"iterations": 9}, {"iterations": -1}, {"width": 0}, {"height": 0}, {"normal_squarings": 11},
                                 {"sigma_color": -1.0}, {"sigma_plane": float("nan")}, {"albedo_floor": float("inf")},
                                 {"flags": RT_PROFILE}, {"flags": RT_DN_NO_DEMODULATE | RT_ADAPTIVE}])
def test_denoise_refuses_values_outside_their_range(bad):
    assert _denoise(_dn(**bad)) == RT_E_INVALID


def test_denoise_refuses_a_sample_count_below_one():
    assert _denoise(_dn(), spp=0) == RT_E_INVALID


def test_render_guides_refuses_null_buffers_and_other_flags(eng):
    guides = np.zeros((H, W, RT_GUIDE_DOUBLES))
    cam = ctypes.byref(eng.cam.c)
    assert lib.rt_render_guides(eng._scene, cam, ctypes.byref(eng.params()), None, None) == RT_E_INVALID
    assert lib.rt_render_guides(None, cam, ctypes.byref(eng.params()), _ptr(guides), None) == RT_E_INVALID
    assert lib.rt_render_guides(eng._scene, None, ctypes.byref(eng.params()), _ptr(guides), None) == RT_E_INVALID
    assert lib.rt_render_guides(eng._scene, cam, None, _ptr(guides), None) == RT_E_INVALID
    for flags in (RT_PROFILE, RT_SPLIT_SHADE, RT_ADAPTIVE, RT_PARALLEL_IMAGES, RT_DN_NO_DEMODULATE):
        assert lib.rt_render_guides(eng._scene, cam, ctypes.byref(eng.params(flags=flags)), _ptr(guides), None) == RT_E_INVALID, flags
    p = eng.params()
    p.width = 0
    assert lib.rt_render_guides(eng._scene, cam, ctypes.byref(p), _ptr(guides), None) == RT_E_INVALID
    p = eng.params(band_rows=2, band_count=2, band_index=2)
    assert lib.rt_render_guides(eng._scene, cam, ctypes.byref(p), _ptr(guides), None) == RT_E_INVALID


def test_render_denoised_refuses_partial_frames_odd_spp_and_other_modes(eng):
    rgb = np.zeros((H, W, 3), np.uint8)
    cam = ctypes.byref(eng.cam.c)
    st = rt_stats()

    def call(p, dn=None, out=rgb):
        return lib.rt_render_denoised(eng._scene, cam, ctypes.byref(p), ctypes.byref(dn) if dn is not None else None,
                                      _ptr(out) if out is not None else None, None, ctypes.byref(st))

    assert call(eng.params(), out=None) == RT_E_INVALID
    for spp in (1, 3, 7):
        p = eng.params()
        p.spp = spp
        assert call(p) == RT_E_INVALID, spp
        assert "even" in lib.rt_last_error().decode()
    assert call(eng.params(flags=RT_ADAPTIVE)) == RT_E_INVALID
    assert call(eng.params(flags=RT_PARALLEL_IMAGES)) == RT_E_INVALID
    assert call(eng.params(band_rows=2, band_count=2, band_index=0)) == RT_E_INVALID
    assert call(eng.params(), _dn(iterations=9)) == RT_E_INVALID
    assert call(eng.params(), _dn(flags=RT_PROFILE)) == RT_E_INVALID
    p = eng.params()
    p.width = 0
    assert call(p) == RT_E_INVALID


def test_python_wrappers_refuse_mismatched_buffers(eng):
    acc = np.zeros((H, W, 3))
    with pytest.raises(ValueError):
        art.denoise(acc, acc, 2, np.zeros((H, W, 4)))  # guides too small
    with pytest.raises(ValueError):
        art.denoise(acc.astype(np.float32), acc, 2, np.zeros((H, W, RT_GUIDE_DOUBLES)))
    with pytest.raises(art.RTError) as e:
        art.denoise(acc, acc, 2, np.zeros((H, W, RT_GUIDE_DOUBLES)), iterations=9)
    assert e.value.code == RT_E_INVALID
    assert RT_OUT_DEVICE == 1  # RT_DN_NO_DEMODULATE shares rt_denoise_params.flags with it
    assert RT_DN_NO_DEMODULATE & 127 == 0  # and collides with no rt_params flag


def test_the_new_kernels_are_in_the_library_and_spill_nothing():
    ks = kernel_resources.kernels(os.path.join(ROOT, "another_raytracer_amd", "libart.so"))
    guides = {n: k for n, k in ks.items() if "k_guides" in n}
    atrous = {n: k for n, k in ks.items() if "k_dn_atrousILi" in n}
    tiled = {n: k for n, k in ks.items() if "k_dn_atrous_ldsILi" in n}
    assert len(guides) >= 4 and any("Lb1E" in n for n in guides)  # spheres (LDS image and HBM), mesh, all features
    assert len(atrous) == 8 and len(tiled) == 2  # tap spacings 1 .. 128 with direct loads, 1 and 2 from an LDS tile
    assert any("k_dn_prepare" in n for n in ks) and any("k_dn_finish" in n for n in ks)
    for n, k in ks.items():
        if "k_guides" in n or "k_dn_" in n:
            assert k.get(".vgpr_spill_count", 0) == 0, (n, k.get(".vgpr_spill_count"))
