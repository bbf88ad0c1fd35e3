"""The image-texel calls at the C ABI boundary and in the wrappers, host only (rt_scene_images_get,
rt_scene_texture_images_get, rt_scene_texels_get, rt_scene_update_texels, rt_radiance_grad_texels): declarations and
bindings, every refusal before a device is touched, the getters against rt_tex_image's inputs, the C++ facade, and the
texel kernels' presence and register budgets in libart.so."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd.rays import _native_scene
from another_raytracer_amd._lib import RT_GLOBAL_SCENE, RT_OK, RT_OUT_DEVICE, RT_PROFILE, lib, rt_radiance_params, rt_stats, rt_update_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

RT_E_INVALID, RT_E_DEVICE = -1, -3
NEW = ("rt_scene_images_get", "rt_scene_texture_images_get", "rt_scene_texels_get", "rt_scene_update_texels", "rt_radiance_grad_texels")
N = 67
IMG_A = (np.arange(4 * 3 * 3, dtype=np.uint8).reshape(3, 4, 3) * 7 + 16)     # h 3, w 4, bpp 3
IMG_B = (np.arange(2 * 5 * 4, dtype=np.uint8).reshape(5, 2, 4) * 5 + 20)     # h 5, w 2, bpp 4


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def built():
    """A caller-built scene: image A on a rect, a solid sphere, image B (bpp 4) barycentric on a triangle."""
    art.reset_scene_rng()
    w = art.hittable_list()
    ta, tb = art.image_texture(IMG_A), art.image_texture(IMG_B)
    solid = art.solid_color(0.5, 0.25, 0.75)
    bary = art.barycentric_image_texture((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), tb)
    w.add(art.xy_rect(-1.0, 1.0, -1.0, 1.0, 0.0, art.lambertian(ta)))
    w.add(art.sphere((0.0, 3.0, 0.0), 1.0, art.lambertian(solid)))
    w.add(art.triangle((3.0, 0.0, 0.0), (4.0, 0.0, 0.0), (3.0, 1.0, 0.0), art.lambertian(bary)))
    world = art.hittable_list(native=art.compile_world(w, 0))
    return world, (ta.id, tb.id, solid.id, bary.id)


@pytest.fixture(scope="module")
def capsule():
    return art.scene_manager().build("9")


# ------------------------------------------------------------------------------------------------ declarations
def test_the_five_functions_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "art.h")).read()
    declared = set(re.findall(r"\b(rt_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    nm = subprocess.run(["nm", "-D", "--defined-only", art._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in declared and f" T {name}\n" in nm and name in art._lib.SIGNATURES, name
    assert set(declared) == set(art._lib.SIGNATURES)
    restype, argtypes = art._lib.SIGNATURES["rt_radiance_grad_texels"]
    assert restype is ctypes.c_int and len(argtypes) == 12  # rt_radiance_grad's eleven and grad_texels before stats
    assert argtypes[:10] == art._lib.SIGNATURES["rt_radiance_grad"][1][:10] and argtypes[11] == ctypes.POINTER(rt_stats)
    assert art._lib.SIGNATURES["rt_scene_update_texels"][1][1] == ctypes.POINTER(rt_update_params)
    assert re.search(r"#define RT_ABI_VERSION 5\b", header)  # additive
    for name in ("scene_images", "scene_texels", "update_texels"):
        assert name in art.__all__ and callable(getattr(art, name))
    assert art.get_option("grad.texel_copies") == 0


@pytest.mark.parametrize("bad", [-1, 65, 0.5])
def test_the_copies_option_has_a_range(options, bad):
    for v in (0, 1, 64):
        options("grad.texel_copies", v)
        assert art.get_option("grad.texel_copies") == v
    with pytest.raises(art.RTError):
        options("grad.texel_copies", bad)


# ------------------------------------------------------------------------------------------------ the getters
def test_getters_on_a_caller_built_scene_return_what_rt_tex_image_took(built):
    world, (ta, tb, solid, bary) = built
    desc, first, tex = art.scene_images(world)
    assert desc.dtype == np.int32 and first.dtype == np.int64 and tex.dtype == np.int32
    assert desc.tolist() == [[4, 3, 3], [2, 5, 4]]          # creation order, {w, h, bpp}
    assert first.tolist() == [0, 12]                         # prefix sums of w * h
    T, td = art.scene_textures(world)
    assert len(tex) == len(T)
    want = np.full(len(T), -1, np.int32)
    want[[ta, tb, bary]] = [0, 1, 1]
    assert tex.tolist() == want.tolist() and tex[solid] == -1
    assert (td[tex >= 0, 0] >= 3).all() and (td[tex < 0, 0] < 3).all()  # exactly the image and barycentric image textures
    a, b = art.scene_texels(world, 0), art.scene_texels(world, 1)
    assert a.dtype == np.uint8 and a.shape == (3, 4, 3) and b.shape == (5, 2, 4)
    assert np.array_equal(a, IMG_A) and np.array_equal(b, IMG_B)
    with pytest.raises(IndexError):
        art.scene_texels(world, 2)
    with pytest.raises(IndexError):
        art.scene_texels(world, -1)


def test_getters_on_the_capsule_scene(capsule):
    desc, first, tex = art.scene_images(capsule)
    assert len(desc) >= 1 and (desc[:, :2] > 0).all() and ((desc[:, 2] >= 1) & (desc[:, 2] <= 4)).all()
    texels = desc[:, 0].astype(np.int64) * desc[:, 1]
    assert first.tolist() == [0] + np.cumsum(texels)[:-1].tolist()
    _, td = art.scene_textures(capsule)
    assert len(tex) == len(td) and ((tex >= 0) == (td[:, 0] >= 3)).all() and tex.max() == len(desc) - 1
    assert (td[:, 0] == 4).any()  # the capsule's appearance is a barycentric image
    px = art.scene_texels(capsule, 0)
    assert px.shape == (desc[0, 1], desc[0, 0], desc[0, 2]) and px.max() > px.min()
    # the raw calls: counts with NULL outs, capacities checked
    h = _native_scene(capsule)
    assert lib.rt_scene_images_get(h, None, None, 0) == len(desc)
    assert lib.rt_scene_texture_images_get(h, None, 0) == len(tex)
    assert lib.rt_scene_texels_get(h, 0, None, 0) == px.nbytes
    small = np.zeros(3, np.int32)
    assert lib.rt_scene_images_get(h, _ptr(small), None, 0) == RT_E_INVALID
    assert lib.rt_scene_texture_images_get(h, _ptr(small), len(tex) - 1) == RT_E_INVALID
    assert lib.rt_scene_texels_get(h, 0, _ptr(np.zeros(16, np.uint8)), 16) == RT_E_INVALID
    assert lib.rt_scene_texels_get(h, len(desc), None, 0) == RT_E_INVALID and lib.rt_scene_texels_get(h, -1, None, 0) == RT_E_INVALID
    for fn, args in ((lib.rt_scene_images_get, (None, None, 0)), (lib.rt_scene_texture_images_get, (None, 0)), (lib.rt_scene_texels_get, (0, None, 0))):
        assert fn(None, *args) == RT_E_INVALID and len(lib.rt_last_error()) > 0


# ------------------------------------------------------------------------------------------------ rt_scene_update_texels
def _update(world, image=0, first_row=0, n_rows=1, scene=True, params=True, buf=True, ms=False, **fields):
    u = rt_update_params()
    for k, v in fields.items():
        setattr(u, k, v)
    b = np.zeros(4096, np.uint8)
    t = ctypes.c_double(-1.0)
    rc = lib.rt_scene_update_texels(_native_scene(world) if scene else None, ctypes.byref(u) if params else None, image, _ptr(b) if buf else None,
                                    first_row, n_rows, ctypes.byref(t) if ms else None)
    return rc, t.value


def test_update_refusals_come_before_any_device_work(built):
    world, _ = built

    def refused(**kw):
        return _update(world, **kw)[0] == RT_E_INVALID and len(lib.rt_last_error()) > 0
    assert refused(scene=False) and refused(params=False)
    assert refused(image=-1) and refused(image=2) and refused(image=1 << 20)
    assert refused(first_row=-1) and refused(first_row=3, n_rows=1) and refused(first_row=2, n_rows=2) and refused(n_rows=-1)
    assert refused(first_row=4, n_rows=0)                       # a range that starts beyond the image, even when empty
    assert refused(image=1, first_row=0, n_rows=6)
    assert refused(first_row=1 << 62, n_rows=1 << 62)           # must not wrap
    assert refused(buf=False)
    assert refused(flags=RT_PROFILE) and refused(flags=RT_GLOBAL_SCENE | RT_OUT_DEVICE) and refused(stream=1234)
    assert b"rows" in lib.rt_last_error() or b"stream" in lib.rt_last_error()


def test_an_empty_update_is_ok_and_touches_no_device(built):
    world, _ = built
    assert _update(world, n_rows=0) == (RT_OK, -1.0)
    assert _update(world, n_rows=0, ms=True) == (RT_OK, 0.0)
    assert _update(world, first_row=3, n_rows=0, buf=False)[0] == RT_OK       # the end of the image, no buffer
    assert _update(world, image=1, first_row=5, n_rows=0, flags=RT_OUT_DEVICE, stream=1234)[0] == RT_OK
    assert np.array_equal(art.scene_texels(world, 0), IMG_A)


@pytest.mark.skipif(lib.rt_device_count() > 0, reason="checks the no-device failure path")
def test_a_valid_update_without_a_device_fails_loudly(built):
    world, _ = built
    assert _update(world, n_rows=3)[0] == RT_E_DEVICE
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.update_texels(world, 0, IMG_A)


def test_update_wrapper_checks_dtype_shape_and_stride(built):
    world, _ = built
    good = np.array(IMG_A)
    for bad in (good.astype(np.int8), good.astype(np.float64), good[:, :3], good[:, :, :2], good.reshape(3, 12), np.zeros((3, 8, 3), np.uint8)[:, ::2],
                np.zeros((2, 5, 4), np.uint8)):
        with pytest.raises(ValueError):
            art.update_texels(world, 0, bad)
    with pytest.raises(TypeError):
        art.update_texels(world, 0, good.tolist())
    with pytest.raises(IndexError):
        art.update_texels(world, 2, good)
    with pytest.raises(ValueError):
        art.update_texels(world, 0, good, stream=1234)   # a stream belongs to device tensors
    with pytest.raises(art.RTError, match="RT_E_INVALID"):
        art.update_texels(world, 0, good, first_row=1)   # three rows from row 1 of three
    import torch
    with pytest.raises(ValueError):
        art.update_texels(world, 0, torch.from_numpy(good))  # a tensor, but on the host
    assert art.update_texels(world, 0, good[:0]) is None     # no rows: nothing happens


# ------------------------------------------------------------------------------------------------ rt_radiance_grad_texels
def _grad(world, n=N, scene=True, params=True, rays=True, weights=True, radiance=True, grads=True, texels=True, stats=False, **fields):
    m = max(1, min(n, 64))  # (a refused call reads nothing)
    r, w, out = np.zeros((m, 7)), np.zeros((m, 3)), np.zeros((m, 3))
    gt, gm, gb, gx = np.zeros((4096, 4)), np.zeros((4096, 5)), np.zeros(3), np.zeros((64, 3))
    q = rt_radiance_params(max_depth=50)
    for k, v in fields.items():
        setattr(q, k, v)
    st = rt_stats()
    g = (_ptr(gt), _ptr(gm), _ptr(gb)) if grads else (None, None, None)
    return lib.rt_radiance_grad_texels(_native_scene(world) if scene else None, ctypes.byref(q) if params else None, _ptr(r) if rays else None, None,
                                       _ptr(w) if weights else None, n, _ptr(out) if radiance else None, *g, _ptr(gx) if texels else None,
                                       ctypes.byref(st) if stats else None)


def test_grad_refusals_are_rt_radiance_grads(built):
    world, _ = built

    def refused(**kw):
        return _grad(world, **kw) == RT_E_INVALID and len(lib.rt_last_error()) > 0
    assert refused(scene=False) and refused(params=False) and refused(rays=False) and refused(weights=False)
    assert refused(weights=False, radiance=False, grads=False, texels=False)   # a refusal comes before "nothing asked for"
    assert refused(n=-1) and refused(n=(1 << 30) + 1)
    assert b"rt_radiance_grad_texels" in lib.rt_last_error()
    assert refused(n=1 << 30, spp=3) and b"kMaxPassSlots" in lib.rt_last_error()
    for flag in (RT_PROFILE, 8, 16, 32, 64, 512):
        assert refused(flags=flag) and refused(flags=flag | RT_OUT_DEVICE)
    assert refused(max_depth=0) and refused(spp=-1) and refused(stream=1234)
    assert refused(id_base=(1 << 32) - N + 1) and refused(id_base=(1 << 64) - 1)


@pytest.mark.parametrize("fields", [{}, {"flags": RT_OUT_DEVICE}, {"flags": RT_GLOBAL_SCENE, "spp": 8}, {"flags": RT_OUT_DEVICE, "stream": 1234}])
def test_zero_rays_or_no_output_is_ok_and_touches_no_device(built, fields):
    world, _ = built
    assert _grad(world, n=0, **fields) == RT_OK
    assert _grad(world, n=0, rays=False, weights=False, radiance=False, grads=False, texels=False, stats=True, **fields) == RT_OK
    assert _grad(world, radiance=False, grads=False, texels=False, **fields) == RT_OK     # all five outputs NULL
    assert _grad(world, radiance=False, grads=False, texels=False, stats=True, **fields) == RT_OK


@pytest.mark.skipif(lib.rt_device_count() > 0, reason="checks the no-device failure path")
def test_a_valid_grad_call_without_a_device_fails_loudly(built):
    world, _ = built
    assert _grad(world) == RT_E_DEVICE
    assert _grad(world, radiance=False, grads=False) == RT_E_DEVICE   # the texel output alone is an output
    assert _grad(world, texels=False) == RT_E_DEVICE                  # and so are the others without it
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.radiance_grad(world, np.zeros((N, 7)), np.zeros((N, 3)), texels=True)


def test_the_row_limit_of_a_vertex_record():
    pytest.skip("T + M + 1 + N >= 2^32 needs a scene with four thousand million texels (12 GB of bytes through rt_tex_image): the image counts of a "
                "compiled scene cannot be faked from outside the library, so the refusal is read in abi.cpp (radiance_grad) only")


def test_grad_wrappers_check_their_buffers(built):
    world, _ = built
    rays, w = np.zeros((N, 7)), np.zeros((N, 3))
    for bad in (rays.astype(np.float32), np.zeros((N, 6)), np.zeros((N, 14))[:, ::2]):
        with pytest.raises(ValueError):
            art.radiance_grad(world, bad, w, texels=True)
    for bad in (w.astype(np.float32), np.zeros((N + 1, 3)), np.zeros((N, 6))[:, ::2]):
        with pytest.raises(ValueError):
            art.radiance_grad(world, rays, bad, texels=True)
    cam = art.camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 16 / 9, 0.0, 5.0)
    with pytest.raises(ValueError):
        art.render_grad(world, cam, 16, 9, 2, np.zeros((9, 16, 4)), texels=True)
    import torch
    t_rays = torch.zeros((N, 7), dtype=torch.float64)
    for bad in ({0: torch.zeros((4, 3, 3))}, {0: torch.zeros((3, 4, 4))}, {0: torch.zeros((3, 4, 3), dtype=torch.uint8)}, {0: np.zeros((3, 4, 3))}):
        with pytest.raises(ValueError):
            art.differentiable_radiance(world, t_rays, texels=bad)
    with pytest.raises(IndexError):
        art.differentiable_radiance(world, t_rays, texels={2: torch.zeros((3, 4, 3))})


# ------------------------------------------------------------------------------------------------ the C++ facade
def test_the_cpp_facade_compiles(tmp_path):
    src = tmp_path / "q.cpp"
    src.write_text("""
#include "art_engine.hpp"
int main() {
    art::scene_manager sm("assets");
    art::scene world = sm.build("4");
    const int n = 32;
    std::vector<std::int64_t> first;
    std::vector<std::int32_t> desc = art::scene_images(world, &first);
    std::vector<std::uint8_t> px = art::scene_texels(world, 0);
    art::update_texels(world, 0, px.data(), 0, desc[1]);
    double ms = 0;
    art::update_texels(world, 0, px.data(), 1, 2, RT_OUT_DEVICE, nullptr, &ms);
    std::vector<double> rays(7 * n), w(3 * n, 1.0), radiance(3 * n), gt(4 * 64), gm(5 * 64), gb(3), gx(3 * desc[0] * desc[1]);
    art::radiance_options o;
    o.max_depth = 3;
    rt_stats st{};
    art::radiance_grad(world, rays.data(), w.data(), n, radiance.data(), gt.data(), gm.data(), gb.data(), gx.data(), o, nullptr, &st);
    art::radiance_grad(world, rays.data(), w.data(), n, nullptr, nullptr, nullptr, nullptr, gx.data());
    art::radiance_grad(world, rays.data(), w.data(), n, nullptr, nullptr, nullptr, gb.data());  // the call without texels stays
    return first.empty() ? 1 : 0;
}
""")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


# ------------------------------------------------------------------------------------------------ the kernels
def test_the_texel_kernels_are_in_the_library_and_meet_their_register_budgets():
    ks = kernel_resources.kernels(os.path.join(ROOT, "another_raytracer_amd", "libart.so"))
    texel = {n: k for n, k in ks.items() if "k_texel_grad" in n}
    # the forms whose textures include an image: all textures on the three HBM-scene feature sets, barycentric images on
    # the two with triangles -- no solid / checker form
    assert len(texel) == 5, sorted(texel)
    assert sum("Lj15E" in n for n in texel) == 3 and sum("Lj19E" in n for n in texel) == 2
    for n, k in texel.items():
        # three waves per SIMD: 512 / 3 = 168 VGPRs (AGPRs included), 256-lane blocks, no static LDS
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 168 and k[".max_flat_workgroup_size"] == 256, (n, k)
        assert k[".group_segment_fixed_size"] == 0, (n, k)
    found = [k for n, k in ks.items() if "k_texel_finish" in n]
    assert len(found) == 1 and found[0][".vgpr_count"] + found[0].get(".agpr_count", 0) <= 168 and found[0].get(".vgpr_spill_count", 0) == 0
    assert sum("k_radiance_grad" in n for n in ks) == 8 and sum("k_grad_finish" in n for n in ks) == 1
