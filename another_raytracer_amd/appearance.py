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
import numpy as np

from . import _update

MATERIAL_DOUBLES, TEXTURE_DOUBLES = 5, 4   # art.h RT_MATERIAL_DOUBLES, RT_TEXTURE_DOUBLES


def scene_materials(world):
    """rt_scene_materials_get: (params, desc) -- params (M, 5) float64: albedo r, g, b; fuzz; ir as the scene holds them
    now (a field the material's type does not use as the host record holds it); desc (M, 2) int32: type (0 lambertian,
    1 metal, 2 dielectric, 3 diffuse_light, 4 isotropic), texture id or -1.  Row k is the material with id k.  Needs no
    device unless the scene has been updated."""
    return _update.get(world, "scene_materials", ((MATERIAL_DOUBLES,), np.float64), ((2,), np.int32))


def scene_textures(world):
    """rt_scene_textures_get: (params, desc) -- params (T, 4) float64: colour r, g, b; scale; desc (T, 3) int32: type
    (0 solid, 1 checker, 2 noise, 3 image, 4 barycentric image), a checker's even and odd texture ids (-1, -1 otherwise).
    Row k is the texture with id k.  Needs no device unless the scene has been updated."""
    return _update.get(world, "scene_textures", ((TEXTURE_DOUBLES,), np.float64), ((3,), np.int32))


def update_materials(world, m, first=0, stream=None, timing=False):
    """rt_scene_update_materials: m holds rows (albedo r, g, b; fuzz; ir) for materials [first, first + n), shape (n, 5)
    float64 in scene_materials' order.  A metal takes albedo and fuzz (stored as min(fuzz, 1)), a dielectric ir; a
    lambertian, a diffuse_light and an isotropic take nothing -- update their texture.

    m, stream and timing are update_spheres': a numpy array copies and blocks (a non-finite value anywhere in a row is
    refused), a contiguous float64 torch tensor on the scene's device is read in place on `stream` (default: torch's current
    stream) and is not inspected; timing=True returns the device time in milliseconds."""
    return _update.update(world, m, "m", ((MATERIAL_DOUBLES,),), "shape (n, 5): albedo r, g, b; fuzz; ir per material", "update_materials", first, stream, timing)


def update_textures(world, t, first=0, stream=None, timing=False):
    """rt_scene_update_textures: t holds rows (colour r, g, b; scale) for textures [first, first + n), shape (n, 4) float64
    in scene_textures' order.  A solid_color takes the colour, a noise_texture the scale (its perlin table stays); checker,
    image and barycentric image textures take nothing.  Every material that uses the texture -- directly or through a
    checker -- shows the new value.  t, stream and timing as update_materials."""
    return _update.update(world, t, "t", ((TEXTURE_DOUBLES,),), "shape (n, 4): colour r, g, b; scale per texture", "update_textures", first, stream, timing)
