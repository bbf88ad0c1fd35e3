"""The refusal ladder of rt_scene_update_triangles, _spheres, _materials and _textures as one table: every row is refused
by every one of the four with RT_E_INVALID and a message, before a device is touched; an empty update in range is RT_OK
with *ms == 0.  (tests/test_update_api.py, test_update_spheres_api.py and test_update_materials_api.py hold each
function's own cases and the message texts.)  Host-only."""
import ctypes

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import RT_OUT_DEVICE, lib, rt_update_params

RT_OK, RT_E_INVALID = 0, -1
KINDS = {"triangles": (lib.rt_scene_update_triangles, lib.rt_scene_triangles_get, 9, 1), "spheres": (lib.rt_scene_update_spheres, lib.rt_scene_spheres_get, 4, 1),
         "materials": (lib.rt_scene_update_materials, lib.rt_scene_materials_get, 5, 2), "textures": (lib.rt_scene_update_textures, lib.rt_scene_textures_get, 4, 2)}


@pytest.fixture(scope="module")
def world():
    """Six triangles and five spheres over four materials and three textures."""
    art.reset_scene_rng()
    mats = [art.lambertian((0.5, 0.5, 0.5)), art.lambertian(art.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))), art.metal((0.7, 0.6, 0.5), 0.25),
            art.dielectric(1.5)]
    w = art.hittable_list()
    w.add(art.bvh_node([art.triangle((k, 0.0, -k), (k + 1.0, 0.25 * k, -k), (k, 1.0, 0.5 - k), mats[k % 4]) for k in range(6)]))
    for k in range(5):
        w.add(art.sphere((2.0 * k, 0.5, 3.0), 0.5, mats[k % 4]))
    return art.compile_world(w, 0)


def count_of(world, kind):
    get, outs = KINDS[kind][1], KINDS[kind][3]
    return get(world, *(None,) * outs, 0)


def call(world, kind, v="ok", first=0, n=None, scene=True, params=True, **fields):
    """The kind's update of rows [first, first + n) (default: all of v, which defaults to positive finite values for the
    whole scene); returns (the return code, *ms, which starts at -1)."""
    fn, width = KINDS[kind][0], KINDS[kind][2]
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


def with_value(where, bad):
    """A full buffer with `bad` as its first, a middle or its last value."""
    def kw(count, width):
        v = np.arange(1.0, width * count + 1.0).reshape(count, width)
        v.flat[{"first": 0, "middle": (width * count) // 2, "last": width * count - 1}[where]] = bad
        return {"v": v}
    return kw


def as_int32(bits):
    return bits - (1 << 32) if bits >= 1 << 31 else bits


LADDER = {"NULL scene": {"scene": False}, "NULL params": {"params": False}, "NULL buffer with n > 0": {"v": None, "n": 1},
          "negative first": {"first": -1, "n": 1}, "negative n": {"n": -1}, "first + n overflows": {"first": 1 << 62, "n": 1 << 62},
          "stream without RT_OUT_DEVICE": {"stream": 1234}}
for bit in range(32):
    if 1 << bit != RT_OUT_DEVICE:
        LADDER[f"flag bit {bit}"] = {"flags": as_int32(1 << bit)}
        LADDER[f"flag bit {bit} with RT_OUT_DEVICE"] = {"flags": as_int32(1 << bit | RT_OUT_DEVICE)}
for name, bad in (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
    for where in ("first", "middle", "last"):
        LADDER[f"{name} as the {where} value"] = with_value(where, bad)


@pytest.mark.parametrize("row", list(LADDER))
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_update_function_refuses_every_row_of_the_ladder(world, kind, row):
    kw = LADDER[row]
    if callable(kw):
        kw = kw(count_of(world, kind), KINDS[kind][2])
    lib.rt_scene_triangles_get(None, None, 0)  # leaves another call's message behind: the refusal must set its own
    stale = lib.rt_last_error()
    rc, _ = call(world, kind, **kw)
    assert rc == RT_E_INVALID
    assert len(lib.rt_last_error()) > 0 and lib.rt_last_error() != stale


@pytest.mark.parametrize("kind", list(KINDS))
def test_an_empty_update_in_range_is_ok_with_zero_ms(world, kind):
    count = count_of(world, kind)
    assert count > 0
    for first in (0, count // 2, count):
        assert call(world, kind, n=0, first=first) == (RT_OK, 0.0)
        assert call(world, kind, v=None, n=0, first=first) == (RT_OK, 0.0)
    assert call(world, kind, n=0, flags=RT_OUT_DEVICE, stream=1234) == (RT_OK, 0.0)
