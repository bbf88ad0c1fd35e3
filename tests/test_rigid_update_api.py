"""rt_scene_update_rects, rt_scene_update_boxes, rt_scene_update_objects and their getters without a device: the exports
and bindings, the whole refusal ladder of tests/test_update_refusals.py, the getters of a never-uploaded scene (the
constructor arguments bit for bit, the pinned object order of translate(rotate_y(box)) and of a constant_medium over it),
the helpers rotation and medium_density against what a compile makes, the Python wrappers' buffer checks, the C++ facade
and the new kernels' resources.  Host-only."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd import _lib
from another_raytracer_amd._lib import RT_OUT_DEVICE, lib, rt_update_params
from tests.test_update_refusals import LADDER
from tests.update_common import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_OK, RT_E_INVALID, RT_E_DEVICE = 0, -1, -3
KINDS = {"rects": (lib.rt_scene_update_rects, lib.rt_scene_rects_get, 5), "boxes": (lib.rt_scene_update_boxes, lib.rt_scene_boxes_get, 6),
         "objects": (lib.rt_scene_update_objects, lib.rt_scene_objects_get, 4)}
PY = {"rects": (art.update_rects, art.scene_rects, 5, 2), "boxes": (art.update_boxes, art.scene_boxes, 6, 1), "objects": (art.update_objects, art.scene_objects, 4, 4)}
SYMBOLS = ("rt_scene_update_rects", "rt_scene_update_boxes", "rt_scene_update_objects", "rt_scene_rects_get", "rt_scene_boxes_get", "rt_scene_objects_get")
PRIM, BVH, TRANSLATE, ROTATE_Y, MEDIUM = range(5)
RECT, BOX = 2 << 30, 3 << 30  # primitive references: type << 30 | index

# the small world's values: nothing round, so a swapped or narrowed field shows
RECTS = np.array([[0.1, 5.3, -0.7, 4.9, 7.25], [-1.3, 2.1, 0.3, 3.7, -0.45], [0.9, 1.7, -2.3, 2.9, 11.0 / 3.0]])  # xy, xz loose; yz in the bvh_node
BOXES = np.array([[0.1, 0.2, 0.3, 1.7, 3.3, 1.9], [-2.1, 0.0, 0.7, -0.3, 1.0 / 3.0, 2.9], [4.1, 0.0, 4.3, 5.2, 1.1, 5.9], [6.1, 0.2, 4.7, 7.3, 0.9, 6.4]])
ANGLES, OFFSETS = (15.0, -18.0), np.array([[1.3, 0.0, 2.95], [-2.6, 0.1, 0.65]])
DENSITY = 0.35


class World:
    """Two loose rects, translate(rotate_y(box)), constant_medium(translate(rotate_y(box))) and a bvh_node of two boxes and a
    rect: ten objects, three rects, four boxes."""

    def __init__(self):
        art.reset_scene_rng()
        self.mats = [art.lambertian((0.7, 0.3, 0.3)), art.metal((0.7, 0.6, 0.5), 0.25), art.diffuse_light(art.solid_color(4.0, 4.0, 4.0))]
        m = self.mats
        w = art.hittable_list()
        w.add(art.xy_rect(*RECTS[0], m[0]))
        w.add(art.xz_rect(*RECTS[1], m[2]))
        w.add(art.translate(art.rotate_y(art.box(tuple(BOXES[0, :3]), tuple(BOXES[0, 3:]), m[1]), ANGLES[0]), tuple(OFFSETS[0])))
        self.medium = art.constant_medium(art.translate(art.rotate_y(art.box(tuple(BOXES[1, :3]), tuple(BOXES[1, 3:]), m[0]), ANGLES[1]), tuple(OFFSETS[1])),
                                          DENSITY, (0.9, 0.9, 0.9))
        w.add(self.medium)
        w.add(art.bvh_node([art.box(tuple(BOXES[2, :3]), tuple(BOXES[2, 3:]), m[0]), art.yz_rect(*RECTS[2], m[1]),
                            art.box(tuple(BOXES[3, :3]), tuple(BOXES[3, 3:]), m[1])]))
        self.handle = art.compile_world(w, 0)


@pytest.fixture(scope="module")
def hw():
    return World()


@pytest.fixture(scope="module")
def world(hw):
    return hw.handle


def count_of(world, kind):
    return KINDS[kind][1](world, None, None, 0)


def call(world, kind, v="ok", first=0, n=None, scene=True, params=True, **fields):
    """tests/test_update_refusals.py's call for the three new kinds: (the return code, *ms, which starts at -1)."""
    fn, _, width = KINDS[kind]
    count = count_of(world, kind)
    if isinstance(v, str):
        v = np.arange(1.0, width * count + 1.0).reshape(count, width)
    u = rt_update_params()
    for k, val in fields.items():
        setattr(u, k, val)
    ms = ctypes.c_double(-1.0)
    rc = fn(world if scene else None, ctypes.byref(u) if params else None, None if v is None else ctypes.c_void_p(v.ctypes.data), first,
            (0 if v is None else len(v)) if n is None else n, ctypes.byref(ms))
    return rc, ms.value


def test_the_symbols_are_declared_exported_and_bound():
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "art.h")).read()
    for s in SYMBOLS:
        assert f" T {s}\n" in nm and s in _lib.SIGNATURES and f"{s}(rt_scene* scene" in header, s
    for f in ("scene_rects", "scene_boxes", "scene_objects", "update_rects", "update_boxes", "update_objects", "rotation", "medium_density"):
        assert callable(getattr(art, f)) and f in art.__all__
    assert "#define RT_RECT_DOUBLES   5" in header and "#define RT_BOX_DOUBLES    6" in header and "#define RT_OBJECT_DOUBLES 4" in header
    assert (art.OBJ_PRIM, art.OBJ_BVH, art.OBJ_TRANSLATE, art.OBJ_ROTATE_Y, art.OBJ_MEDIUM) == (0, 1, 2, 3, 4)
    assert lib.rt_abi_version() == 5  # the addition is additive


# ------------------------------------------------------------------------------------------------ 1. refusals
@pytest.mark.parametrize("row", list(LADDER))
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_new_update_function_refuses_every_row_of_the_ladder(world, kind, row):
    kw = LADDER[row]
    if callable(kw):
        kw = kw(count_of(world, kind), KINDS[kind][2])
    lib.rt_scene_triangles_get(None, None, 0)  # leaves another call's message behind: the refusal must set its own
    stale = lib.rt_last_error()
    rc, _ = call(world, kind, **kw)
    assert rc == RT_E_INVALID
    assert len(lib.rt_last_error()) > 0 and lib.rt_last_error() != stale and f"rt_scene_update_{kind}".encode() in lib.rt_last_error()


@pytest.mark.parametrize("kind", list(KINDS))
def test_an_empty_update_in_range_is_ok_with_zero_ms(world, kind):
    count = count_of(world, kind)
    assert count == {"rects": 3, "boxes": 4, "objects": 10}[kind]
    for first in (0, count // 2, count):
        assert call(world, kind, n=0, first=first) == (RT_OK, 0.0)
        assert call(world, kind, v=None, n=0, first=first) == (RT_OK, 0.0)
    assert call(world, kind, n=0, flags=RT_OUT_DEVICE, stream=1234) == (RT_OK, 0.0)
    assert PY[kind][0](world, np.zeros((0, KINDS[kind][2]))) is None and PY[kind][0](world, np.zeros((0, KINDS[kind][2])), timing=True) == 0.0


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_range_beyond_the_count_is_refused_with_the_count(world, kind):
    count, width = count_of(world, kind), KINDS[kind][2]
    for first, n in ((count, 1), (count - 1, 2), (count + 1, 0), (0, count + 1)):
        rc, _ = call(world, kind, v=np.ones((count + 1, width)), first=first, n=n)
        assert rc == RT_E_INVALID and f"{count} {kind}".encode() in lib.rt_last_error()


@pytest.mark.parametrize("kind", list(KINDS))
def test_getters_take_either_pointer_and_refuse_a_short_cap(world, kind):
    get, width, dw = KINDS[kind][1], KINDS[kind][2], PY[kind][3]
    count = count_of(world, kind)
    v, d = np.full((count, width), -7.0), np.full((count, dw), -7, np.int32)
    vp, dp = ctypes.c_void_p(v.ctypes.data), ctypes.c_void_p(d.ctypes.data)
    assert get(world, vp, None, count) == count and get(world, None, dp, count + 3) == count
    both_v, both_d = PY[kind][1](world)
    assert (bits(v) == bits(both_v)).all() and (d == both_d).all()
    assert get(None, None, None, 0) == RT_E_INVALID and get(None, vp, dp, count) == RT_E_INVALID
    for short in (0, count - 1, -1):
        assert get(world, vp, None, short) == RT_E_INVALID and get(world, None, dp, short) == RT_E_INVALID
        assert f"rt_scene_{kind}_get".encode() in lib.rt_last_error()


@pytest.mark.skipif(lib.rt_device_count() > 0, reason="checks the no-device failure path")
@pytest.mark.parametrize("kind", list(KINDS))
def test_valid_calls_without_a_device_fail_loudly(world, kind):
    assert call(world, kind)[0] == RT_E_DEVICE  # the arguments passed every check
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        PY[kind][0](world, PY[kind][1](world)[0])


# ------------------------------------------------------------------------------------------------ 2. getters
def test_rects_and_boxes_of_a_never_uploaded_scene_are_the_constructor_arguments(hw, world):
    m = [x.id for x in hw.mats]
    r, rd = art.scene_rects(world)
    assert r.dtype == np.float64 and r.shape == (3, 5) and rd.dtype == np.int32 and rd.shape == (3, 2)
    assert (bits(r) == bits(RECTS)).all()  # compiled order: the world list walked in order
    assert rd.tolist() == [[0, m[0]], [1, m[2]], [2, m[1]]]  # axis: xy, xz, yz; the material ids
    b, bd = art.scene_boxes(world)
    assert b.shape == (4, 6) and bd.shape == (4, 1) and (bits(b) == bits(BOXES)).all()
    assert bd[:, 0].tolist() == [m[1], m[0], m[0], m[1]]


def test_object_order_and_desc_are_pinned(hw, world):
    """A wrapper is numbered after what it wraps: translate(rotate_y(box)) is box, rotate_y, translate; a constant_medium over
    such a chain comes last.  Only world-level objects have a world slot."""
    p, d = art.scene_objects(world)
    assert p.dtype == np.float64 and p.shape == (10, 4) and d.dtype == np.int32 and d.shape == (10, 4)
    iso = int(d[8, 2])
    want = [[PRIM, RECT | 0, 0, 0], [PRIM, RECT | 1, 0, 1],
            [PRIM, BOX | 0, 0, -1], [ROTATE_Y, 2, 0, -1], [TRANSLATE, 3, 0, 2],
            [PRIM, BOX | 1, 0, -1], [ROTATE_Y, 5, 0, -1], [TRANSLATE, 6, 0, -1], [MEDIUM, 7, iso, 3],
            [BVH, int(d[9, 1]), -1, 4]]
    assert d.astype(np.int64).tolist() == [[x if x < 2 ** 31 else x - 2 ** 32 for x in row] for row in want]
    # the medium's phase material is the isotropic one the medium made, an ordinary row of scene_materials
    mdesc = art.scene_materials(world)[1]
    assert mdesc[iso, 0] == 4 and iso not in [x.id for x in hw.mats]
    assert d[9, 1] >= 0  # the BVH's root node
    want_p = np.zeros((10, 4))
    for k, (tr, ro) in enumerate(((4, 3), (7, 6))):
        want_p[tr, :3] = OFFSETS[k]
        want_p[ro, :2] = art.rotation(ANGLES[k])
    want_p[8, 0] = art.medium_density(DENSITY)
    assert (bits(p) == bits(want_p)).all()
    assert (bits(p[4, :3]) == bits(OFFSETS[0])).all() and p[8, 0] == -1.0 / DENSITY


# ------------------------------------------------------------------------------------------------ 3. helpers
ANGLE_LIST = [-180.0 + 7.5 * k for k in range(49)] + [15.0, -18.0, 0.1]


def test_rotation_gives_the_bits_a_compile_gives():
    art.reset_scene_rng()
    m = art.lambertian((0.5, 0.5, 0.5))
    w = art.hittable_list()
    for a in ANGLE_LIST:
        w.add(art.rotate_y(art.box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), m), a))
    p, d = art.scene_objects(art.compile_world(w, 0))
    turns = np.flatnonzero(d[:, 0] == ROTATE_Y)
    assert len(turns) == len(ANGLE_LIST) == 52 and (d[turns, 3] == np.arange(52)).all()
    got = np.array([art.rotation(a) for a in ANGLE_LIST])
    assert (bits(got) == bits(p[turns, :2])).all()
    assert art.rotation(0.0) == (0.0, 1.0) and art.rotation(90.0)[0] == 1.0
    # degrees * pi / 180.0 in that order: math.radians multiplies by pi / 180 and differs in the last bit for some angles
    assert any(art.rotation(a) != (math.sin(math.radians(a)), math.cos(math.radians(a))) for a in ANGLE_LIST)


def test_medium_density_gives_the_bits_a_compile_gives():
    art.reset_scene_rng()
    m = art.lambertian((0.5, 0.5, 0.5))
    densities = [0.01, 0.2, 0.0001, 0.35, 3.0, 1.0 / 3.0]
    w = art.hittable_list()
    for k, dens in enumerate(densities):
        w.add(art.constant_medium(art.sphere((3.0 * k, 0.0, 0.0), 1.0, m), dens, (1.0, 1.0, 1.0)))
    p, d = art.scene_objects(art.compile_world(w, 0))
    media = np.flatnonzero(d[:, 0] == MEDIUM)
    assert len(media) == len(densities)
    assert (bits(np.array([art.medium_density(x) for x in densities])) == bits(p[media, 0])).all()


# ------------------------------------------------------------------------------------------------ 4. the Python wrappers
@pytest.mark.parametrize("kind", list(KINDS))
def test_python_wrappers_refuse_wrong_buffers_and_arguments(world, kind):
    import torch
    update, get, width, _ = PY[kind]
    count = count_of(world, kind)
    for bad in (np.zeros((count, width), np.float32), np.zeros((count, width - 1)), np.zeros((count, width + 1)), np.zeros(width * count),
                np.zeros((count, 2 * width))[:, ::2], np.zeros((count, width, 1)), np.zeros((count, width), np.int64)):
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
        get(None)
    with pytest.raises(TypeError):
        get(art.hittable_list())


def test_the_cpp_facade_compiles_and_links(tmp_path):
    src = tmp_path / "u.cpp"
    src.write_text("""
#include "art_engine.hpp"
int main() {
    art::scene_manager sm("assets");
    art::scene world = sm.build("6");
    std::vector<std::int32_t> rdesc, bdesc, odesc;
    std::vector<double> r = art::scene_rects(world, &rdesc), b = art::scene_boxes(world, &bdesc), o = art::scene_objects(world, &odesc);
    for (std::size_t k = 0; k < o.size() / RT_OBJECT_DOUBLES; ++k)
        if (odesc[4 * k] == RT_OBJ_TRANSLATE) o[RT_OBJECT_DOUBLES * k] += 10.0;
    for (std::size_t k = 0; k < r.size() / RT_RECT_DOUBLES; ++k)
        if (rdesc[2 * k] == 1) r[RT_RECT_DOUBLES * k + 4] -= 1.0;
    double ms = 0;
    art::update_objects(world, o.data(), 0, static_cast<std::int64_t>(o.size() / RT_OBJECT_DOUBLES));
    art::update_rects(world, r.data(), 0, static_cast<std::int64_t>(r.size() / RT_RECT_DOUBLES), 0, nullptr, &ms);
    art::update_boxes(world, b.data() + RT_BOX_DOUBLES, 1, 1);
    return ms >= 0 && art::scene_boxes(world).size() == b.size() && bdesc.size() * RT_BOX_DOUBLES == b.size() ? 0 : 1;
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
        assert f"U {s}\n" in nm, s


def test_the_new_kernels_are_built_and_keep_their_values_in_registers():
    """k_update_rects, k_update_boxes and k_update_objects in the built code object: no spill, no scratch, no LDS."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels(os.path.join(ROOT, "another_raytracer_amd", "libart.so"))
    for name in ("k_update_rects", "k_update_boxes", "k_update_objects"):
        mine = [k for n, k in ks.items() if name in n]
        assert len(mine) == 1, (name, sorted(ks))
        k = mine[0]
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0 and k[".group_segment_fixed_size"] == 0, (name, k)
