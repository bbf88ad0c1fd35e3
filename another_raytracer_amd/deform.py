"""Deforming a compiled scene (rt_scene_update_triangles, include/art.h): new vertices for its triangles and a refit of
its BVH boxes on the device -- an animated mesh, a morph target, vertices that come out of a torch optimiser -- where a
new scene would cost a graph, a full SAH build and an upload per frame.

    world = art.scene_manager().build("cow")
    P = art.scene_triangles(world)                   # (n, 3, 3) float64, the compiled order
    art.update_triangles(world, P + [0.0, 1.0, 0.0])  # numpy: copies and blocks
    V = torch.from_numpy(P).cuda()
    art.update_triangles(world, deform(V))           # a device tensor: in place on torch's current stream, no wait
    frames = art.render_views(world, cams, W, H, spp, out=frames_gpu)   # same stream: ordered after the update

Every later call on the scene gives the bits a scene compiled fresh from the same vertices gives (closest hits do not
depend on the tree); topology, materials and texture coordinates stay.
"""
import ctypes

import numpy as np

from . import _update
from ._lib import check, lib
from .rays import _native_scene

# layout.h BvhNode as uploaded: the four child boxes as planes, the 32-bit child codes, the 16-bit codes in pad
BVH_NODE = np.dtype([("lox", "<f4", 4), ("hix", "<f4", 4), ("loy", "<f4", 4), ("hiy", "<f4", 4), ("loz", "<f4", 4), ("hiz", "<f4", 4),
                     ("child", "<i4", 4), ("pad", "<i4", 4)])
assert BVH_NODE.itemsize == 128


def scene_triangles(world):
    """rt_scene_triangles_get: the scene's triangles as it holds them now, (n, 3, 3) float64 -- triangle, vertex (pt1, pt2,
    pt3), xyz -- in compiled order: the order the triangles are met walking the world list.  Takes a scene_manager scene,
    its .objects or a compile_world handle.  Needs no device unless the scene has been updated."""
    return _update.get(world, "scene_triangles", ((3, 3), np.float64))[0]


def update_triangles(world, p, first=0, stream=None, timing=False):
    """rt_scene_update_triangles: p holds new vertices for triangles [first, first + n), shape (n, 3, 3) or (n, 9) float64 in
    scene_triangles' order; every BVH box is then refitted on the device.

    p: a numpy array (the call copies through the scene's workspace and blocks), or a contiguous float64 torch tensor on the
    scene's device, read in place on `stream` (a torch stream or a raw hipStream_t; default: torch's current stream) -- the
    call then returns once the work is enqueued, unless timing is asked for.  The update writes the arrays the render
    kernels read: order the calls on one scene on one stream, or synchronise between them.  timing=True returns the
    device time of the update's kernels in milliseconds (HIP events; waits), otherwise None."""
    return _update.update(world, p, "p", ((3, 3), (9,)), "shape (n, 3, 3) or (n, 9): three vertices per triangle", "update_triangles", first, stream, timing)


def scene_spheres(world):
    """rt_scene_spheres_get: the scene's spheres as it holds them now, (n, 4) float64 -- cx, cy, cz, r; center0 for a
    moving_sphere -- in compiled order: the order the spheres are met walking the world list.  Needs no device unless the
    scene has been updated."""
    return _update.get(world, "scene_spheres", ((4,), np.float64))[0]


def update_spheres(world, s, first=0, stream=None, timing=False):
    """rt_scene_update_spheres: s holds new (cx, cy, cz, r) for spheres [first, first + n), shape (n, 4) float64 in
    scene_spheres' order; every BVH box, and the LDS scene image of a scene that runs out of one, is then refitted on the
    device.  Materials stay, and so does a moving sphere's motion: it translates with it.

        S = art.scene_spheres(world)
        S[1:, 1] += 0.1 * np.sin(t + S[1:, 0])            # bounce
        art.update_spheres(world, S)

    s, stream and timing are update_triangles': a numpy array copies and blocks (a non-finite value or a radius <= 0 is
    refused), a contiguous float64 torch tensor on the scene's device is read in place on `stream` and is not inspected."""
    return _update.update(world, s, "s", ((4,),), "shape (n, 4): cx, cy, cz, r per sphere", "update_spheres", first, stream, timing)


def scene_lds_image(world, rebuilt=False):
    """rt_scene_lds_image_get (diagnostic): the scene's LDS scene image (csrc/layout.h) followed by its tile representatives
    as uint8, or None when the scene has no image.  rebuilt=False: the device's bytes as they are now; rebuilt=True: what
    the host builder makes now of the scene as the device holds it -- the same bytes after any update.  Uploads the scene
    if needed; blocks."""
    handle = _native_scene(world)
    n = check(lib.rt_scene_lds_image_get(handle, int(bool(rebuilt)), None, 0), "scene_lds_image")
    if n == 0:
        return None
    out = np.zeros((n,), np.uint8)
    check(lib.rt_scene_lds_image_get(handle, int(bool(rebuilt)), ctypes.c_void_p(out.ctypes.data), n), "scene_lds_image")
    return out


def scene_bvh(world):
    """rt_scene_bvh_get (diagnostic): the device's BVH as it is now -- (nodes, primrefs): a structured array of the 128-byte
    four-child nodes (BVH_NODE: lox, hix, loy, hiy, loz, hiz as float32[4] planes of the child boxes; child: int32[4],
    >= 0 an inner node, -1 empty, else a leaf ~((count << 24) | first slot); pad: the 16-bit codes) and the uint32 primitive
    reference of every leaf slot (type << 30 | index; type 1 = triangle).  Uploads the scene if needed; blocks."""
    handle = _native_scene(world)
    nn, nr = ctypes.c_int64(), ctypes.c_int64()
    check(lib.rt_scene_bvh_get(handle, None, 0, None, 0, ctypes.byref(nn), ctypes.byref(nr)), "scene_bvh")
    nodes = np.zeros((nn.value,), BVH_NODE)
    refs = np.zeros((nr.value,), np.uint32)
    check(lib.rt_scene_bvh_get(handle, ctypes.c_void_p(nodes.ctypes.data), nn.value, ctypes.c_void_p(refs.ctypes.data), nr.value, None, None),
          "scene_bvh")
    return nodes, refs
