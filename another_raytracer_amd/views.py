"""Many cameras of one scene in one call (rt_render_views, include/art.h): an orbit of a mesh for a multi-view dataset,
the six faces of a cube-map probe, a light field.

    world = art.scene_manager().build("cow")
    cams = [art.camera(eye, world.lookat, (0, 1, 0), world.vfov, W / H, 0.0, 10.0) for eye in orbit]
    frames = art.render_views(world, cams, W, H, spp=16)             # (V, H, W, 3) uint8, frame v == engine.run with cams[v]

Every view is one frame of engine.run bit for bit; the views share one persistent launch instead of paying a workspace
reset, the launches, a wait and a copy each.  Small frames gain the most (64 views of 128 x 128 x 16: 0.13-0.19 of the
loop's time); at 1920 x 1080 a loop of engine.run is as fast or faster.
"""
import ctypes

import numpy as np

from ._buffers import address, is_tensor, same_place, scene_background, stream_handle
from ._lib import RT_FP64, RT_GLOBAL_SCENE, RT_OUT_DEVICE, check, lib, rt_camera, rt_params, rt_stats
from .rays import _native_scene


def render_views(world_or_objects, cams, width, height, spp, max_depth=50, seed=0, seeds=None, background=None, global_scene=False,
                 accum=False, out=None, stream=None, stats=False):
    """rt_render_views over a compiled scene (a scene_manager().build(...) scene, its .objects, or what compile_world
    returns): len(cams) frames of width x height, spp samples per pixel, view v through cams[v] (art.camera) with seed
    seeds[v] (seeds None: `seed` for every view).  Frame v equals engine.run with that camera and seed bit for bit.

    Returns the (V, H, W, 3) uint8 frames; with accum, also the (V, H, W, 3) float64 radiance sums; with stats=True, also a
    dict (segments, primary, ms, passes = launches of the path kernel): frames, (frames, sums), (frames, stats) or
    (frames, sums, stats).  background None: the scene's own.

    Buffers: by default numpy arrays (the call copies and blocks).  out: the frames' buffer, and accum may be the sums'
    buffer instead of True -- numpy arrays, or contiguous tensors on the scene's device, which are written in place on
    `stream` (a torch stream or a raw hipStream_t; default: torch's current stream) without waiting unless stats is
    asked for.  Calls on one scene share its workspace: order them on one stream, or synchronise between them.
    Every view has the same size, samples and depth; a frame of more than 2^31 paths takes engine.run, which splits it
    into passes."""
    handle = _native_scene(world_or_objects)
    cams = list(cams)
    for c in cams:
        if not hasattr(c, "c"):
            raise TypeError("cams must be a sequence of art.camera")
    nviews = len(cams)
    width, height, spp = int(width), int(height), int(spp)
    if spp < 1:
        raise ValueError("spp must be >= 1")
    if seeds is not None:
        seeds = [int(x) for x in seeds]
        if len(seeds) != nviews:
            raise ValueError(f"seeds must hold one seed per camera ({nviews}), or be None")
    shape = (nviews, height, width, 3)
    want_accum = accum is not False and accum is not None
    acc = None if not want_accum or accum is True else accum
    # buffers that are not given are allocated where the given ones live
    if any(is_tensor(b) for b in (out, acc)):
        import torch
        tdev = next(b.device for b in (out, acc) if is_tensor(b))
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=tdev)
        if want_accum and acc is None:
            acc = torch.empty(shape, dtype=torch.float64, device=tdev)
    else:
        if out is None:
            out = np.empty(shape, np.uint8)
        if want_accum and acc is None:
            acc = np.empty(shape, np.float64)
    out_ptr, out_dev = address(out, "out", ("uint8",), shape=shape, device_index=handle.device)
    acc_ptr, acc_dev = address(acc, "accum", ("float64",), shape=shape, device_index=handle.device) if want_accum else (None, None)
    same_place(out=out_dev, accum=acc_dev)
    background = scene_background(world_or_objects, handle, background)
    p = rt_params()
    p.width, p.height, p.spp, p.max_depth, p.seed, p.fp_mode = width, height, spp, int(max_depth), int(seed), RT_FP64
    p.band_rows, p.band_count, p.band_index = height, 1, 0
    p.flags = (RT_OUT_DEVICE if out_dev else 0) | (RT_GLOBAL_SCENE if global_scene else 0)
    for c in range(3):
        p.background[c] = float(background[c])
    p.stream = stream_handle(stream, out.device if out_dev else None)
    table = (rt_camera * max(nviews, 1))(*[c.c for c in cams])
    seed_arr = None if seeds is None else (ctypes.c_uint64 * max(nviews, 1))(*seeds)
    st = rt_stats()
    check(lib.rt_render_views(handle, table, seed_arr, nviews, ctypes.byref(p), ctypes.c_void_p(out_ptr),
                              ctypes.c_void_p(acc_ptr) if acc_ptr else None, ctypes.byref(st) if stats else None), "render_views")
    result = (out,) + ((acc,) if want_accum else ())
    if stats:
        result += ({"segments": st.segments, "primary": st.primary, "ms": st.ms, "passes": st.passes},)
    return result[0] if len(result) == 1 else result
