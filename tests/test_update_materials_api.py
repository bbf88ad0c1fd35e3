"""rt_scene_update_materials, rt_scene_update_textures, rt_scene_materials_get, rt_scene_textures_get: the exports and
their bindings, the index rule (a compiled index is the graph's id: the Python objects' .id), the getters without a
device, every refusal (each happens before a device is touched, with a message), the Python wrappers' buffer checks, the
C++ facade and the new kernels' resources.  Host-only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd import _lib
from another_raytracer_amd.scene import scene_dump
from another_raytracer_amd._lib import RT_GLOBAL_SCENE, RT_OUT_DEVICE, RT_PROFILE, lib, rt_scene_info, rt_update_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_OK, RT_E_INVALID, RT_E_DEVICE = 0, -1, -3
SYMBOLS = ("rt_scene_update_materials", "rt_scene_update_textures", "rt_scene_materials_get", "rt_scene_textures_get")
LAMBERTIAN, METAL, DIELECTRIC, LIGHT, ISOTROPIC = range(5)
SOLID, CHECKER, NOISE, IMAGE, BARY = range(5)


class World:
    """One of each material and texture type, a constant_medium included."""

    def __init__(self):
        art.reset_scene_rng()
        self.red = art.solid_color(0.8, 0.25, 0.125)
        self.even, self.odd = art.solid_color(0.2, 0.3, 0.1), art.solid_color(0.9, 0.9, 0.9)
        self.checker = art.checker_texture(self.even, self.odd)
        self.noise = art.noise_texture(4.0)
        self.image = art.image_texture(np.arange(8 * 8 * 3, dtype=np.uint8).reshape(8, 8, 3))
        self.bary = art.barycentric_image_texture((0, 0), (1, 0), (0, 1), self.image)
        self.lamb = art.lambertian(self.red)
        self.lamb_checker = art.lambertian(self.checker)
        self.lamb_noise = art.lambertian(self.noise)
        self.lamb_image = art.lambertian(self.image)
        self.lamb_bary = art.lambertian(self.bary)
        self.metal = art.metal((0.7, 0.6, 0.5), 0.25)
        self.metal_rough = art.metal((0.5, 0.5, 0.25), 3.0)  # stored as 1 (material.h:47)
        self.glass = art.dielectric(1.5)
        self.emit = art.solid_color(4.0, 3.0, 2.0)
        self.light = art.diffuse_light(self.emit)
        self.fog = art.solid_color(0.75, 0.75, 1.0)
        w = art.hittable_list()
        mats = [self.lamb, self.lamb_checker, self.lamb_noise, self.lamb_image, self.metal, self.metal_rough, self.glass, self.light]
        w.add(art.bvh_node([art.sphere((2.0 * k, 0.5, 0.0), 0.5, m) for k, m in enumerate(mats)]))
        w.add(art.triangle((0, 0, 5), (1, 0, 5), (0, 1, 5), self.lamb_bary))
        n_before = 9
        w.add(art.constant_medium(art.sphere((0.0, 3.0, 0.0), 1.0, self.lamb), 0.25, self.fog))
        self.isotropic_id = n_before  # the medium's isotropic material: made when the medium is, after the nine above
        self.handle = art.compile_world(w, 0)


@pytest.fixture(scope="module")
def hw():
    return World()


@pytest.fixture(scope="module")
def world(hw):
    return hw.handle


NM, NT = 10, 9


def _update(world, what="materials", v="ok", first=0, n=None, scene=True, params=True, ms=False, **fields):
    fn, width = (lib.rt_scene_update_materials, 5) if what == "materials" else (lib.rt_scene_update_textures, 4)
    count = NM if what == "materials" else NT
    if isinstance(v, str):
        v = np.arange(1.0, width * count + 1.0).reshape(count, width)
    u = rt_update_params()
    for k, val in fields.items():
        setattr(u, k, val)
    t = ctypes.c_double(-1.0)
    return fn(world if scene else None, ctypes.byref(u) if params else None, None if v is None else ctypes.c_void_p(v.ctypes.data),
              first, (0 if v is None else len(v)) if n is None else n, ctypes.byref(t) if ms else None)


def _refused(world, **kw):
    return _update(world, **kw) == RT_E_INVALID and len(lib.rt_last_error()) > 0


BOTH = pytest.mark.parametrize("what", ["materials", "textures"])


def test_the_symbols_are_declared_exported_and_bound():
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "art.h")).read()
    for s in SYMBOLS:
        assert f" T {s}\n" in nm and s in _lib.SIGNATURES and f"{s}(rt_scene* scene" in header, s
    for f in ("scene_materials", "scene_textures", "update_materials", "update_textures"):
        assert callable(getattr(art, f)) and f in art.__all__
    assert "#define RT_MATERIAL_DOUBLES 5" in header and "#define RT_TEXTURE_DOUBLES  4" in header
    assert lib.rt_abi_version() == 5  # the addition is additive


def test_indices_are_the_graphs_ids_and_counts_are_scene_infos(hw, world):
    info = rt_scene_info()
    assert lib.rt_scene_info_get(world, ctypes.byref(info)) == RT_OK
    assert lib.rt_scene_materials_get(world, None, None, 0) == info.materials == NM
    assert lib.rt_scene_textures_get(world, None, None, 0) == info.textures == NT
    m, md = art.scene_materials(world)
    t, td = art.scene_textures(world)
    assert m.shape == (NM, 5) and m.dtype == np.float64 and md.shape == (NM, 2) and md.dtype == np.int32
    assert t.shape == (NT, 4) and t.dtype == np.float64 and td.shape == (NT, 3) and td.dtype == np.int32
    # textures by .id: colour, scale; {type, even, odd}
    assert (t[hw.red.id] == (0.8, 0.25, 0.125, 0.0)).all() and tuple(td[hw.red.id]) == (SOLID, -1, -1)
    assert (t[hw.even.id, :3] == (0.2, 0.3, 0.1)).all() and (t[hw.odd.id, :3] == (0.9, 0.9, 0.9)).all()
    assert tuple(td[hw.checker.id]) == (CHECKER, hw.even.id, hw.odd.id)
    assert t[hw.noise.id, 3] == 4.0 and tuple(td[hw.noise.id]) == (NOISE, -1, -1)
    assert tuple(td[hw.image.id]) == (IMAGE, -1, -1) and tuple(td[hw.bary.id]) == (BARY, -1, -1)
    assert (t[hw.emit.id, :3] == (4.0, 3.0, 2.0)).all() and (t[hw.fog.id, :3] == (0.75, 0.75, 1.0)).all()
    assert sorted(x.id for x in (hw.red, hw.even, hw.odd, hw.checker, hw.noise, hw.image, hw.bary, hw.emit, hw.fog)) == list(range(NT))
    # materials by .id: albedo, fuzz, ir; {type, tex}
    for mat, tex in ((hw.lamb, hw.red), (hw.lamb_checker, hw.checker), (hw.lamb_noise, hw.noise), (hw.lamb_image, hw.image), (hw.lamb_bary, hw.bary)):
        assert tuple(md[mat.id]) == (LAMBERTIAN, tex.id) and (m[mat.id] == 0.0).all()  # unused fields: as the host record holds them
    assert (m[hw.metal.id] == (0.7, 0.6, 0.5, 0.25, 0.0)).all() and tuple(md[hw.metal.id]) == (METAL, -1)
    assert (m[hw.metal_rough.id] == (0.5, 0.5, 0.25, 1.0, 0.0)).all()  # fuzz 3 was clamped at construction
    assert (m[hw.glass.id] == (0.0, 0.0, 0.0, 0.0, 1.5)).all() and tuple(md[hw.glass.id]) == (DIELECTRIC, -1)
    assert tuple(md[hw.light.id]) == (LIGHT, hw.emit.id)
    assert tuple(md[hw.isotropic_id]) == (ISOTROPIC, hw.fog.id)  # the medium's isotropic is an ordinary entry
    assert sorted([x.id for x in (hw.lamb, hw.lamb_checker, hw.lamb_noise, hw.lamb_image, hw.lamb_bary, hw.metal, hw.metal_rough, hw.glass, hw.light)]
                  + [hw.isotropic_id]) == list(range(NM))


def test_getters_take_either_pointer_and_refuse_a_short_cap(world):
    for fn, count, pw, dw, word in ((lib.rt_scene_materials_get, NM, 5, 2, b"materials"), (lib.rt_scene_textures_get, NT, 4, 3, b"textures")):
        p, d = np.full((count, pw), -7.0), np.full((count, dw), -7, np.int32)
        assert fn(world, ctypes.c_void_p(p.ctypes.data), None, count) == count and (p != -7.0).any()
        assert fn(world, None, ctypes.c_void_p(d.ctypes.data), count + 3) == count and (d != -7).all()
        p2, d2 = np.full((count, pw), -7.0), np.full((count, dw), -7, np.int32)
        assert fn(world, ctypes.c_void_p(p2.ctypes.data), ctypes.c_void_p(d2.ctypes.data), count) == count
        assert (p2 == p).all() and (d2 == d).all()
        p3 = np.full((count, pw), -7.0)
        assert fn(world, ctypes.c_void_p(p3.ctypes.data), None, count - 1) == RT_E_INVALID
        assert str(count).encode() in lib.rt_last_error() and word in lib.rt_last_error() and (p3 == -7.0).all()
        assert fn(world, None, ctypes.c_void_p(d2.ctypes.data), 0) == RT_E_INVALID
        assert fn(None, None, None, 0) == RT_E_INVALID
    one = art.scene_manager().build("1")
    m, md = art.scene_materials(one)
    t, td = art.scene_textures(one)
    assert len(m) == one.info["materials"] > 100 and len(t) == one.info["textures"] > 100
    assert set(md[:, 0]) == {LAMBERTIAN, METAL, DIELECTRIC} and (md[md[:, 0] == LAMBERTIAN, 1] >= 0).all()
    assert set(td[:, 0]) == {SOLID, CHECKER} and (td[td[:, 0] == CHECKER, 1:] >= 0).all()  # the ground is a checker of two solid colours
    assert (m[md[:, 0] == METAL, 3] <= 0.5).all() and (m[md[:, 0] == DIELECTRIC, 4] == 1.5).all()


@BOTH
def test_null_arguments_and_ranges_are_refused(world, what):
    count = NM if what == "materials" else NT
    assert _refused(world, what=what, scene=False)
    assert _refused(world, what=what, params=False)
    assert _refused(world, what=what, v=None, n=1)                       # buffer NULL with n > 0
    assert _refused(world, what=what, first=-1, n=1)
    assert _refused(world, what=what, n=-1)
    assert _refused(world, what=what, first=1)                           # first + n = count + 1
    assert _refused(world, what=what, first=count, n=1)
    assert _refused(world, what=what, first=count + 1, n=0)
    assert _refused(world, what=what, first=1 << 62, n=1 << 62)          # no overflow into range
    assert _refused(world, what=what, n=count + 1)
    assert f"{count} {what}".encode() in lib.rt_last_error()


@BOTH
@pytest.mark.parametrize("flag", [RT_PROFILE, RT_GLOBAL_SCENE, 8, 16, 1024, 1 << 30])
def test_other_flag_bits_are_refused(world, what, flag):
    assert _refused(world, what=what, flags=flag)
    assert _refused(world, what=what, flags=flag | RT_OUT_DEVICE)


@BOTH
def test_a_stream_without_rt_out_device_is_refused(world, what):
    assert _refused(world, what=what, stream=1234)
    assert b"RT_OUT_DEVICE" in lib.rt_last_error()


@BOTH
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_in_a_host_buffer_is_refused_used_or_ignored(hw, world, what, bad):
    count, width, word = (NM, 5, "material") if what == "materials" else (NT, 4, "texture")
    for where in range(width * count):  # every double of every row: most of them are fields the record's type ignores
        v = np.arange(1.0, width * count + 1.0).reshape(count, width)
        v.flat[where] = bad
        assert _refused(world, what=what, v=v)
        assert f"{word} {where // width} ".encode() in lib.rt_last_error()
    # named ones: ir of a metal, albedo of a lambertian; the colour of a checker, the scale of a solid colour
    row, col = {"materials": (hw.metal.id, 4), "textures": (hw.red.id, 3)}[what]
    v = np.ones((1, width))
    v[0, col] = bad
    assert _refused(world, what=what, v=v, first=row)
    row = {"materials": hw.lamb.id, "textures": hw.checker.id}[what]
    v = np.ones((1, width))
    v[0, 0] = bad
    assert _refused(world, what=what, v=v, first=row) and f"{word} {row} ".encode() in lib.rt_last_error()
    v = np.arange(1.0, width * count + 1.0).reshape(count, width)
    v[0, 0] = bad  # a value outside the updated rows is not looked at: the range check refuses this one
    assert _refused(world, what=what, v=v[1:3], first=count - 1) and f"{count} {what}".encode() in lib.rt_last_error()


@BOTH
def test_degenerate_calls_are_ok_and_touch_no_device(world, what):
    # no device on a host-only machine: RT_OK shows the call returned before any device work
    count, width = (NM, 5) if what == "materials" else (NT, 4)
    assert _update(world, what=what, v=None, n=0) == RT_OK
    assert _update(world, what=what, n=0, first=count, ms=True) == RT_OK
    assert _update(world, what=what, n=0, flags=RT_OUT_DEVICE, stream=1234) == RT_OK
    update = art.update_materials if what == "materials" else art.update_textures
    assert update(world, np.zeros((0, width))) is None
    assert scene_dump(art.scene_manager().build("c1"))  # a scene that was never updated still dumps


@pytest.mark.skipif(lib.rt_device_count() > 0, reason="checks the no-device failure path")
def test_valid_calls_without_a_device_fail_loudly(world):
    assert _update(world) == RT_E_DEVICE  # the arguments passed every check
    assert _update(world, what="textures", v=np.ones((2, 4)), first=4, ms=True) == RT_E_DEVICE
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.update_materials(world, art.scene_materials(world)[0])
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.update_textures(world, art.scene_textures(world)[0])


def test_python_wrappers_refuse_wrong_buffers_and_arguments(world):
    import torch
    for update, count, width in ((art.update_materials, NM, 5), (art.update_textures, NT, 4)):
        for bad in (np.zeros((count, width), np.float32), np.zeros((count, width - 1)), np.zeros((count, width + 1)), np.zeros(width * count),
                    np.zeros((count, 2 * width))[:, ::2], np.zeros((count, width, 1))):
            with pytest.raises(ValueError):
                update(world, bad)
        with pytest.raises(TypeError):
            update(world, [[0.5] * width] * count)
        with pytest.raises(ValueError):
            update(world, np.ones((count, width)), stream=1234)  # a stream belongs to device tensors
        with pytest.raises(art.RTError, match="RT_E_INVALID"):
            update(world, np.ones((count, width)), first=1)
        with pytest.raises(art.RTError, match="RT_E_INVALID"):
            update(world, np.full((1, width), np.nan))
        with pytest.raises(TypeError):
            update(art.hittable_list(), np.ones((count, width)))  # not compiled
        with pytest.raises(ValueError):
            update(world, torch.ones((count, width), dtype=torch.float64))  # a tensor, but on the host
    with pytest.raises(TypeError):
        art.scene_materials(None)
    with pytest.raises(TypeError):
        art.scene_textures(art.hittable_list())


def test_the_cpp_facade_compiles_and_links(tmp_path):
    src = tmp_path / "u.cpp"
    src.write_text("""
#include "art_engine.hpp"
int main() {
    art::scene_manager sm("assets");
    art::scene world = sm.build("1");
    std::vector<std::int32_t> mdesc, tdesc;
    std::vector<double> m = art::scene_materials(world, &mdesc), t = art::scene_textures(world, &tdesc);
    for (std::size_t k = 0; k < m.size(); k += RT_MATERIAL_DOUBLES)
        if (mdesc[2 * (k / RT_MATERIAL_DOUBLES)] == RT_MAT_METAL) m[k + 3] = 0.5;
    for (std::size_t k = 0; k < t.size(); k += RT_TEXTURE_DOUBLES)
        if (tdesc[3 * (k / RT_TEXTURE_DOUBLES)] == RT_TEX_SOLID) t[k] *= 0.5;
    double ms = 0;
    art::update_materials(world, m.data(), 0, static_cast<std::int64_t>(m.size() / RT_MATERIAL_DOUBLES));
    art::update_textures(world, t.data() + RT_TEXTURE_DOUBLES, 1, 2, 0, nullptr, &ms);
    return ms >= 0 && art::scene_textures(world).size() == t.size() ? 0 : 1;
}
""")
    # compiled and linked against the built library (not run: main needs a device)
    libdir = os.path.dirname(_lib.LIB_PATH)
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "u"),
                          "-L" + libdir, "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    nm = subprocess.run(["nm", "-u", str(tmp_path / "u")], capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert f"U {s}\n" in nm, s  # the facade's four calls resolve to the library's exports


def test_the_new_kernels_are_built_and_keep_their_values_in_registers():
    """k_update_materials, k_update_textures and k_derive_materials in the built code object: no spill, no scratch, no LDS."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(os.path.join(ROOT, "another_raytracer_amd", "libart.so"))
    for name in ("k_update_materials", "k_update_textures", "k_derive_materials"):
        mine = [k for n, k in ks.items() if name in n]
        assert len(mine) == 1, (name, sorted(ks))
        k = mine[0]
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0 and k[".group_segment_fixed_size"] == 0, (name, k)
