"""rt_render_noise_target: struct layouts, argument checks (every refusal happens before a device is touched), the
Python wrapper's buffer checks, the new kernels' register budgets, and the edge cases of the numpy restatement
(tests/nt_reference.py).  Host-only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import (RT_ADAPTIVE, RT_PARALLEL_IMAGES, RT_SPLIT_SHADE, RT_WAVEFRONT, lib, rt_noise_params, rt_noise_result,
                                        rt_stats)
from tests import nt_reference as nt

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
    e = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=32)
    e.set_scene(world.objects, world.background)
    return e


def test_the_structs_match_the_header(tmp_path):
    src = tmp_path / "nt.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "art.h"', "int main(void) {"]
    for cls in (rt_noise_params, rt_noise_result):
        name = cls.__name__
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "nt"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cls in (rt_noise_params, rt_noise_result):
        name = cls.__name__
        assert int(c[name]) == ctypes.sizeof(cls), name
        for f, _ in cls._fields_:
            assert int(c[f"{name}.{f}"]) == getattr(cls, f).offset, f"{name}.{f}"


def _call(eng, p=None, noise=None, rgb=True, scene=True, cam=True):
    out = np.zeros((H, W, 3), np.uint8)
    st, res = rt_stats(), rt_noise_result()
    p = eng.params() if p is None else p
    return lib.rt_render_noise_target(eng._scene if scene else None, ctypes.byref(eng.cam.c) if cam else None, ctypes.byref(p) if p is not False else None,
                                      ctypes.byref(noise) if noise is not None else None, _ptr(out) if rgb else None, None, None, None,
                                      ctypes.byref(st), ctypes.byref(res))


def _refused(eng, **kw):
    rc = _call(eng, **kw)
    return rc == RT_E_INVALID and len(lib.rt_last_error()) > 0


def test_null_arguments_are_refused(eng):
    assert _refused(eng, rgb=False)
    assert _refused(eng, scene=False)
    assert _refused(eng, cam=False)
    assert _refused(eng, p=False)


@pytest.mark.parametrize("flag", [RT_ADAPTIVE, RT_PARALLEL_IMAGES, RT_WAVEFRONT, RT_SPLIT_SHADE])
def test_other_engine_modes_and_the_wavefront_variants_are_refused(eng, flag):
    p = eng.params(flags=flag)
    if flag == RT_ADAPTIVE:
        p.width, p.height = 24, 12
    assert _refused(eng, p=p, noise=rt_noise_params(min_spp=4))
    assert b"RT_" in lib.rt_last_error()


@pytest.mark.parametrize("bad", [dict(min_spp=1), dict(min_spp=-3), dict(min_spp=33), dict(step_spp=-1), dict(min_spp=4, rel_tol=-0.1),
                                 dict(min_spp=4, rel_tol=float("nan")), dict(min_spp=4, rel_tol=float("inf")), dict(min_spp=4, lum_floor=-1.0),
                                 dict(min_spp=4, lum_floor=float("inf")), dict(min_spp=4, lum_floor=float("nan")), dict(min_spp=4, dilate=2),
                                 dict(min_spp=4, dilate=-1)])
def test_values_outside_their_range_are_refused(eng, bad):
    assert _refused(eng, noise=rt_noise_params(**bad)), bad


def test_the_default_min_spp_must_fit_under_the_cap(eng):
    p = eng.params()
    p.spp = 8  # the default min_spp is 32
    assert _refused(eng, p=p)
    assert b"min_spp" in lib.rt_last_error()
    assert _refused(eng, p=p, noise=rt_noise_params())


def test_dilation_is_refused_on_a_band_partition(eng):
    p = eng.params(band_rows=2, band_count=2, band_index=1)
    assert _refused(eng, p=p, noise=rt_noise_params(min_spp=4, dilate=1))
    assert b"partition" in lib.rt_last_error()


def test_invalid_render_parameters_are_refused(eng):
    p = eng.params()
    p.width = 1
    assert _refused(eng, p=p, noise=rt_noise_params(min_spp=4))
    p = eng.params(band_rows=2, band_count=2, band_index=2)
    assert _refused(eng, p=p, noise=rt_noise_params(min_spp=4))


def test_python_wrapper_refuses_wrong_dtypes_and_shapes(eng):
    rgb = np.zeros((H, W, 3), np.uint8)
    with pytest.raises(ValueError):
        eng.run_noise_target(np.zeros((H, W, 2), np.uint8), min_spp=4)  # too small
    with pytest.raises(ValueError):
        eng.run_noise_target(rgb.astype(np.float32), min_spp=4)
    with pytest.raises(ValueError):
        eng.run_noise_target(rgb, accum=np.zeros((H, W, 3), np.float32), min_spp=4)
    with pytest.raises(ValueError):
        eng.run_noise_target(rgb, accum=np.zeros((H, W, 2)), min_spp=4)
    with pytest.raises(ValueError):
        eng.run_noise_target(rgb, counts=np.zeros((H, W), np.int64), min_spp=4)
    with pytest.raises(ValueError):
        eng.run_noise_target(rgb, counts=np.zeros((H - 1, W), np.int32), min_spp=4)
    with pytest.raises(ValueError):
        eng.run_noise_target(rgb, moments=np.zeros((H, W)), min_spp=4)
    with pytest.raises(ValueError):
        eng.run_noise_target(rgb, moments=np.zeros((H, W, 2), np.float32), min_spp=4)
    with pytest.raises(TypeError):
        eng.run_noise_target(rgb, counts=[0] * (H * W), min_spp=4)
    with pytest.raises(TypeError):
        eng.run_noise_target(rgb, min_spp=4, tolerance=0.1)  # unknown option
    with pytest.raises(art.RTError) as e:
        eng.run_noise_target(rgb, min_spp=1)
    assert e.value.code == RT_E_INVALID
    world = art.scene_manager().build("c1")
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, 2.0, world.aperture, 10.0, 0.0, 1.0)
    ad = art.engine(cam, art.engine_mode.adaptive, width=24, height=12, samples_per_pixel=32)
    ad.set_scene(world.objects, world.background)
    with pytest.raises(ValueError):
        ad.run_noise_target(np.zeros((12, 24, 3), np.uint8), min_spp=4)


def test_the_new_kernels_are_in_the_library_and_spill_nothing():
    ks = kernel_resources.kernels(os.path.join(ROOT, "another_raytracer_amd", "libart.so"))
    mine = {n: k for n, k in ks.items() if "k_nt_" in n}
    for want in ("k_nt_accum_base", "k_nt_accum_list", "k_nt_flag", "k_nt_finalize"):
        assert sum(want in n for n in mine) == 1, (want, sorted(mine))
    assert sum("k_nt_select" in n for n in mine) == 2  # with and without dilation
    for n, k in mine.items():
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (n, k)
        assert k.get(".private_segment_fixed_size", 0) == 0, (n, k)


@pytest.mark.parametrize("extra", [["--gpus", "1"], ["--progressive", "4"], ["--denoise"]])
def test_art_render_refuses_noise_target_with_the_other_drivers(tmp_path, extra):
    exe = os.path.join(ROOT, "another_raytracer_amd", "art_render")
    out = subprocess.run([exe, "c1", "16", "12", "32", str(tmp_path / "o.png"), "--noise-target", "0.05", *extra], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 1 and "--noise-target" in out.stderr and not (tmp_path / "o.png").exists()
    for bad in (["--noise-target", "abc"], ["--noise-target", "0"], ["--min-spp", "8"]):
        out = subprocess.run([exe, "c1", "16", "12", "32", str(tmp_path / "o.png"), *bad], capture_output=True, text=True, timeout=120)
        assert out.returncode == 1 and "noise-target" in out.stderr, bad


def test_the_cpp_facade_compiles(tmp_path):
    src = tmp_path / "nt.cpp"
    src.write_text("""
#include "art_engine.hpp"
int main() {
    art::scene_manager sm("assets");
    art::scene world = sm.build("6");
    art::camera cam(world.lookfrom, world.lookat, art::vec3{{0, 1, 0}}, world.vfov, 4.0 / 3, world.aperture, 10.0, 0.0, 1.0);
    art::render_engine eng(640, 480, cam, art::engine_mode::parallel_stripes, 256);
    eng.set_scene(world, world.background);
    std::vector<std::uint8_t> image(640 * 480 * 3);
    std::vector<std::int32_t> counts(640 * 480);
    rt_noise_params noise{};
    noise.rel_tol = 0.05;
    noise.dilate = 1;
    const rt_noise_result r = eng.run_noise_target(image.data(), noise, counts.data());
    const rt_noise_result d = eng.run_noise_target(image.data());
    return r.rounds >= 0 && d.rounds >= 0 && r.samples >= static_cast<std::uint64_t>(r.converged_pixels) ? 0 : 1;
}
""")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


# ---------------------------------------------------------------------------------------------- the restatement's edge cases
def test_two_samples_is_the_smallest_count_the_test_accepts():
    # samples 1 and 3: mean 2, var = (10 - 4*2) / 1 = 2, se2 = 1; thr = tol * (2 + 0.01)
    assert nt.unconverged(4.0, 10.0, 2, rel_tol=0.4, lum_floor=0.01)       # thr^2 = 0.646 < 1
    assert not nt.unconverged(4.0, 10.0, 2, rel_tol=0.5, lum_floor=0.01)   # thr^2 = 1.010 >= 1
    # two equal samples: var == 0 exactly, converged at any tolerance > 0
    assert not nt.unconverged(1.0, 0.5, 2, rel_tol=1e-9, lum_floor=0.01)


def test_a_slightly_negative_variance_is_clamped_to_zero():
    # three samples of 0.1: S1 and S2 as the kernel accumulates them; S2 - S1*mean rounds below zero
    s1 = (0.1 + 0.1) + 0.1
    s2 = (0.1 * 0.1 + 0.1 * 0.1) + 0.1 * 0.1
    assert s2 - s1 * (s1 / 3.0) < 0.0
    assert not nt.unconverged(s1, s2, 3, rel_tol=1e-12, lum_floor=0.0)
    # and without the clamp the comparison would still hold, but a tolerance of 1e-300 (thr^2 underflows to 0) needs it
    assert not nt.unconverged(s1, s2, 3, rel_tol=1e-300, lum_floor=0.0)


def test_zero_luminance_converges_through_the_floor_and_without_it():
    assert not nt.unconverged(0.0, 0.0, 16)                                  # var 0 <= (0.05 * 0.01)^2
    assert not nt.unconverged(0.0, 0.0, 16, rel_tol=0.05, lum_floor=0.0)     # 0 <= 0
    # one bright sample among 15 black ones: far from converged
    assert nt.unconverged(1.0, 1.0, 16)
    # non-finite sums never converge
    assert nt.unconverged(float("nan"), 1.0, 16) and nt.unconverged(float("inf"), float("inf"), 16)


def test_both_extreme_tolerances():
    s1, s2 = np.array([3.0, 0.5]), np.array([2.0, 0.2])
    assert not nt.unconverged(s1, s2, 8, rel_tol=1e300).any()  # thr^2 = inf
    assert nt.unconverged(s1, s2, 8, rel_tol=1e-300).all()     # thr^2 = 0 < se2


def test_a_one_pixel_wide_image_with_dilation():
    unc = np.zeros((7, 1), bool)
    unc[3, 0] = True
    assert nt.dilate3(unc)[:, 0].tolist() == [False, False, True, True, True, False, False]
    moments = np.zeros((7, 1, 2))
    moments[3, 0] = (1.0, 1.0)  # one bright sample of 16: unconverged; the others are black
    active = np.ones((7, 1), bool)
    assert nt.next_active(active, 16, moments, 32)[:, 0].tolist() == [False, False, False, True, False, False, False]
    assert nt.next_active(active, 16, moments, 32, dilate=True)[:, 0].tolist() == [False, False, True, True, True, False, False]
    # a retired neighbour is not revived, and nothing stays active at the cap
    active[2, 0] = False
    assert nt.next_active(active, 16, moments, 32, dilate=True)[:, 0].tolist() == [False, False, False, True, True, False, False]
    assert not nt.next_active(active, 32, moments, 32, dilate=True).any()
    # an unconverged pixel outside the active set does not keep its neighbours active
    active[:] = True
    active[3, 0] = False
    assert not nt.next_active(active, 16, moments, 32, dilate=True).any()


def test_write_color_uses_every_pixels_own_count():
    acc = np.array([[[4.0, 1.0, 0.0]], [[4.0, 1.0, 1e9]]])
    count = np.array([[16], [4]], np.int32)
    rgb = nt.write_color(acc, count)
    assert rgb.tolist() == [[[128, 64, 0]], [[255, 128, 255]]]
