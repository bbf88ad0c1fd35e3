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

Image textures are bytes, not rows of doubles, and have calls of their own (rt_scene_images_get, rt_scene_texels_get,
rt_scene_update_texels):

    desc, first_texel, texture_image = art.scene_images(world)   # per image {w, h, bpp} and its first global texel
    earth = art.scene_texels(world, 0)                            # (h, w, bpp) uint8, top row first
    earth[:, :, 0] //= 2
    art.update_texels(world, 0, earth)                            # or rows: update_texels(world, 0, earth[10:20], first_row=10)
"""
import ctypes

import numpy as np

from . import _update
from ._lib import check, lib
from .rays import _native_scene

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


def scene_images(world):
    """rt_scene_images_get and rt_scene_texture_images_get: (desc, first_texel, texture_image) -- desc (K, 3) int32: w, h,
    bpp of image k, in the order the scene's images were made; first_texel (K,) int64: the global index of the image's
    texel (0, 0), texel (column i, row j from the top) being first_texel[k] + j * w + i -- the rows of radiance_grad's
    texel gradient; texture_image (T,) int32: the image of texture t (an image or a barycentric image texture), else -1.
    Needs no device."""
    desc, first = _update.get(world, "scene_images", ((3,), np.int32), ((), np.int64))
    tex, = _update.get(world, "scene_texture_images", ((), np.int32))
    return desc, first, tex


def _image_desc(handle, image):
    """(w, h, bpp) of image `image` of the native scene; IndexError for an image the scene does not have."""
    n = check(lib.rt_scene_images_get(handle, None, None, 0), "scene_images")
    if not 0 <= int(image) < n:
        raise IndexError(f"image {image} is not one of the scene's {n} images")
    desc = np.empty((n, 3), np.int32)
    check(lib.rt_scene_images_get(handle, ctypes.c_void_p(desc.ctypes.data), None, n), "scene_images")
    return tuple(int(x) for x in desc[int(image)])


def scene_texels(world, image):
    """rt_scene_texels_get: the bytes of image `image` as the scene holds them now, an (h, w, bpp) uint8 array, top row
    first.  Needs no device unless the scene has been updated."""
    handle = _native_scene(world)
    w, h, bpp = _image_desc(handle, image)
    out = np.empty((h, w, bpp), np.uint8)
    check(lib.rt_scene_texels_get(handle, int(image), ctypes.c_void_p(out.ctypes.data), out.nbytes), "scene_texels")
    return out


def update_texels(world, image, texels, first_row=0, stream=None, timing=False):
    """rt_scene_update_texels: texels holds rows [first_row, first_row + n) of image `image`, shape (n, w, bpp) uint8 in
    scene_texels' layout.  Every later call gives the bits a scene compiled with these bytes gives.  texels, stream and
    timing as update_materials: a numpy array copies and blocks, a contiguous uint8 torch tensor on the scene's device is
    read in place on `stream` (default: torch's current stream); timing=True returns the device time in milliseconds."""
    w, _, bpp = _image_desc(_native_scene(world), image)
    return _update.update(world, texels, "texels", ((w, bpp),), f"shape (n, {w}, {bpp}): rows of image {int(image)}", "update_texels", first_row, stream,
                          timing, dtypes=("uint8",), lead=(int(image),))
