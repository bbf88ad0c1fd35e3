"""Recolouring a compiled scene (rt_scene_update_materials / rt_scene_update_textures, include/art.h): new values for its
materials and textures on the device -- a light an optimiser drives, material parameters for inverse rendering, look-dev
on the material query_rays reported, a flickering emitter across render_views frames -- where a new scene would cost a
graph, a full SAH build and an upload.

    params, desc = art.scene_textures(world)          # (T, 4) float64: colour r, g, b; scale -- row = texture.id
    params[lamp.emit.id, :3] *= 1.5                    # a diffuse_light's colour is its texture's
    art.update_textures(world, params)
    M, _ = art.scene_materials(world)                 # (M, 5) float64: albedo r, g, b; fuzz; ir -- row = material.id
    M[mirror.id, 3] = 0.2
    art.update_materials(world, M[mirror.id:mirror.id + 1], first=mirror.id)

Rows are indexed by the ids the scene classes carry (material.id, texture.id; the isotropic material a constant_medium
makes is a row too), and the material index is query_rays' `mat`.  A record takes what its type uses: a metal albedo and
fuzz (clamped to 1), a dielectric ir, a solid texture its colour, a noise texture its scale; everything else in a row is
ignored and stays, so get -> update changes nothing.  Every later call gives the bits a scene compiled fresh with the
same values gives.
"""
import ctypes

import numpy as np

from ._lib import RT_OUT_DEVICE, check, lib, rt_update_params
from ._buffers import address, stream_handle
from .rays import _native_scene

MATERIAL_DOUBLES, TEXTURE_DOUBLES = 5, 4   # art.h RT_MATERIAL_DOUBLES, RT_TEXTURE_DOUBLES


def _get(world, fn, name, width, desc_width):
    handle = _native_scene(world)
    n = check(fn(handle, None, None, 0), name)
    params, desc = np.empty((n, width), np.float64), np.empty((n, desc_width), np.int32)
    if n:
        check(fn(handle, ctypes.c_void_p(params.ctypes.data), ctypes.c_void_p(desc.ctypes.data), n), name)
    return params, desc


def scene_materials(world):
    """rt_scene_materials_get: (params, desc) -- params (M, 5) float64: albedo r, g, b; fuzz; ir as the scene holds them
    now (a field the material's type does not use as the host record holds it); desc (M, 2) int32: type (0 lambertian,
    1 metal, 2 dielectric, 3 diffuse_light, 4 isotropic), texture id or -1.  Row k is the material with id k.  Needs no
    device unless the scene has been updated."""
    return _get(world, lib.rt_scene_materials_get, "scene_materials", MATERIAL_DOUBLES, 2)


def scene_textures(world):
    """rt_scene_textures_get: (params, desc) -- params (T, 4) float64: colour r, g, b; scale; desc (T, 3) int32: type
    (0 solid, 1 checker, 2 noise, 3 image, 4 barycentric image), a checker's even and odd texture ids (-1, -1 otherwise).
    Row k is the texture with id k.  Needs no device unless the scene has been updated."""
    return _get(world, lib.rt_scene_textures_get, "scene_textures", TEXTURE_DOUBLES, 3)


def _update(world, v, arg, width, what, fn, name, first, stream, timing):
    handle = _native_scene(world)
    if not hasattr(v, "shape"):
        raise TypeError(f"{arg} must be a numpy array or a torch tensor")
    shape = tuple(int(x) for x in v.shape)
    if not (len(shape) == 2 and shape[1] == width):
        raise ValueError(f"{arg} must have shape (n, {width}): {what}")
    ptr, dev = address(v, arg, ("float64",), shape=shape, device_index=handle.device)
    u = rt_update_params()
    u.flags = RT_OUT_DEVICE if dev else 0
    u.stream = stream_handle(stream, v.device if dev else None)
    ms = ctypes.c_double()
    check(fn(handle, ctypes.byref(u), ctypes.c_void_p(ptr), int(first), shape[0], ctypes.byref(ms) if timing else None), name)
    return ms.value if timing else None


def update_materials(world, m, first=0, stream=None, timing=False):
    """rt_scene_update_materials: m holds rows (albedo r, g, b; fuzz; ir) for materials [first, first + n), shape (n, 5)
    float64 in scene_materials' order.  A metal takes albedo and fuzz (stored as min(fuzz, 1)), a dielectric ir; a
    lambertian, a diffuse_light and an isotropic take nothing -- update their texture.

    m, stream and timing are update_spheres': a numpy array copies and blocks (a non-finite value anywhere in a row is
    refused), a contiguous float64 torch tensor on the scene's device is read in place on `stream` (default: torch's current
    stream) and is not inspected; timing=True returns the device time in milliseconds."""
    return _update(world, m, "m", MATERIAL_DOUBLES, "albedo r, g, b; fuzz; ir per material", lib.rt_scene_update_materials, "update_materials",
                   first, stream, timing)


def update_textures(world, t, first=0, stream=None, timing=False):
    """rt_scene_update_textures: t holds rows (colour r, g, b; scale) for textures [first, first + n), shape (n, 4) float64
    in scene_textures' order.  A solid_color takes the colour, a noise_texture the scale (its perlin table stays); checker,
    image and barycentric image textures take nothing.  Every material that uses the texture -- directly or through a
    checker -- shows the new value.  t, stream and timing as update_materials."""
    return _update(world, t, "t", TEXTURE_DOUBLES, "colour r, g, b; scale per texture", lib.rt_scene_update_textures, "update_textures",
                   first, stream, timing)
