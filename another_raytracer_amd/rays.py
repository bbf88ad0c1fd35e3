"""Ray queries on a compiled scene (rt_query_rays, include/art.h): hittable_list::hit(r, 0.001, t_max, rec) for arbitrary
rays through the renderer's own BVH traversal -- the closest hit with the whole hit_record, or any-hit occlusion.

    world = art.scene_manager().build("cow")
    hits = art.query_rays(world.objects, rays)                       # (n, 12) records; hits.t, hits.point, hits.prim ...
    blocked = art.query_rays(world.objects, shadow_rays, t_max=dist, any_hit=True)   # (n,) uint8

    L = art.radiance_rays(world, rays, spp=64)                       # (n, 3): the path-traced radiance sums along the rays
    rays, rng = art.camera_rays(cam, W, H, spp)                      # the renderer's own camera rays and RNG states

Buffers are numpy arrays (host path: the call copies and blocks) or contiguous float64 torch tensors on the scene's device
(used in place, on torch's current stream, without waiting: the result tensor is ordered after the query on that stream
like any torch operation).
"""
import ctypes

import numpy as np

from ._buffers import address, same_place, scene_background, stream_handle
from ._lib import (RT_FP64, RT_GLOBAL_SCENE, RT_HIT_DOUBLES, RT_OUT_DEVICE, RT_Q_ANY_HIT, RT_Q_NO_MEDIA, check, lib, rt_params, rt_query_params,
                   rt_radiance_params, rt_stats)
from .scene import _SceneHandle, hittable_list, scene

# columns of a hit record (RT_HIT_DOUBLES = 12)
HIT_FIELDS = {"t": 0, "normal": slice(1, 4), "point": slice(4, 7), "u": 7, "v": 8, "front_face": 9, "prim": 10, "mat": 11}


class HitRecords:
    """The (n, 12) hit records of art.query_rays and named views into them: t, normal (n, 3), point (n, 3), u, v,
    front_face (1.0 / 0.0), prim (the compiled primitive reference; -1 miss, -2 medium event) and mat (material index; -1
    miss).  `records` is the numpy array or torch tensor itself; a miss has t = +inf."""

    def __init__(self, records):
        self.records = records

    def __getattr__(self, name):
        try:
            return self.records[:, HIT_FIELDS[name]]
        except KeyError:
            raise AttributeError(name) from None

    def __len__(self):
        return int(self.records.shape[0])

    def __array__(self, dtype=None, copy=None):
        a = self.records if isinstance(self.records, np.ndarray) else self.records.cpu().numpy()
        return a if dtype is None else a.astype(dtype)


def _native_scene(objects):
    if isinstance(objects, scene):
        objects = objects.objects
    if isinstance(objects, hittable_list):
        if objects._native is None:
            raise TypeError("query_rays takes a compiled scene: pass compile_world(world, device) for a hittable_list built by hand")
        objects = objects._native
    if not isinstance(objects, _SceneHandle):
        raise TypeError("objects must be scene_manager().build(...).objects or the handle compile_world returns")
    return objects


def _rays(rays, device_index):
    """(n, address, is_device) of an (n, 7) float64 ray buffer: a numpy array, or a tensor on the scene's device."""
    if not hasattr(rays, "shape"):
        raise TypeError("rays must be a numpy array or a torch tensor")
    if len(rays.shape) != 2 or int(rays.shape[1]) != 7:
        raise ValueError("rays must have shape (n, 7): origin, direction, time")
    n = int(rays.shape[0])
    return (n,) + address(rays, "rays", ("float64",), shape=(n, 7), device_index=device_index)


def query_rays(objects, rays, t_max=None, any_hit=False, no_media=False, global_scene=False, out=None, stream=None):
    """rt_query_rays over a compiled scene (scene_manager().build(...).objects, or what compile_world returns).

    rays: (n, 7) float64 {ox, oy, oz, dx, dy, dz, time}; t_max: (n,) float64 or None (+inf): the search interval of ray i
    is [0.001, t_max[i]].  numpy arrays, or contiguous torch tensors on the scene's device -- then the query runs in
    place on `stream` (a torch stream or a raw hipStream_t; default: torch's current stream) and returns without waiting
    (on torch's default stream, whose handle is null, the call waits for the inputs and for the query instead).

    Closest mode returns HitRecords over an (n, 12) array / tensor (`out`, or a new one): t, normal, point, u, v,
    front_face, prim, mat (include/art.h); no_media skips constant_medium objects.  any_hit=True returns an (n,) uint8
    array / tensor: 1 where some non-medium primitive lies in the interval.  global_scene forces the HBM traversal on a
    scene that has an LDS image (A/B, tests)."""
    handle = _native_scene(objects)
    n, rays_ptr, dev = _rays(rays, handle.device)
    tmax_ptr, tmax_dev = (None, None) if t_max is None else address(t_max, "t_max", ("float64",), shape=(n,), device_index=handle.device)
    if dev:
        import torch
    if any_hit:
        if out is None:
            out = torch.empty((n,), dtype=torch.uint8, device=rays.device) if dev else np.empty((n,), np.uint8)
        out_ptr, out_dev = address(out, "out", ("uint8", "bool"), shape=(n,), device_index=handle.device)
    else:
        if out is None:
            out = (torch.empty((n, RT_HIT_DOUBLES), dtype=torch.float64, device=rays.device) if dev
                   else np.empty((n, RT_HIT_DOUBLES), np.float64))
        out_ptr, out_dev = address(out, "out", ("float64",), shape=(n, RT_HIT_DOUBLES), device_index=handle.device)
    same_place(rays=dev, t_max=tmax_dev, out=out_dev)
    q = rt_query_params()
    q.flags = ((RT_OUT_DEVICE if dev else 0) | (RT_GLOBAL_SCENE if global_scene else 0) | (RT_Q_ANY_HIT if any_hit else 0)
               | (RT_Q_NO_MEDIA if no_media else 0))
    q.stream = stream_handle(stream, rays.device if dev else None)
    hits_arg = None if any_hit else ctypes.c_void_p(out_ptr)
    occ_arg = ctypes.c_void_p(out_ptr) if any_hit else None
    check(lib.rt_query_rays(handle, ctypes.byref(q), ctypes.c_void_p(rays_ptr), None if tmax_ptr is None else ctypes.c_void_p(tmax_ptr),
                            n, hits_arg, occ_arg), "query_rays")
    return out if any_hit else HitRecords(out)


def radiance_rays(objects, rays, spp=1, max_depth=50, seed=0, sample_base=0, id_base=0, rng=None, background=None, global_scene=False,
                  out=None, stream=None, stats=False):
    """rt_radiance_rays over a compiled scene (a scene_manager().build(...) scene, its .objects, or what compile_world
    returns): the path-traced radiance that arrives along caller-given rays -- other camera models, light probes,
    lightmap texels, several cameras in one launch.

    rays: (n, 7) float64 {ox, oy, oz, dx, dy, dz, time}.  Ray i starts spp paths; path (i, s) runs the renderer's
    _ray_color (miss: background; diffuse_light: emission; otherwise scatter while depth + 1 < max_depth) on the PCG state
    rng[i * spp + s] when rng is given (n * spp states: a uint64 array, or an int64 / uint64 device tensor), else on the
    stream keyed (seed, id_base + i, sample_base + s).  Returns the (n, 3) float64 sums over the samples, in sample order
    from +0.0 (`out`, or a new array / tensor) -- sums as engine.run's accum, not means; with stats=True, (sums, dict)
    with segments, primary and ms.  background None: the scene's own.  Buffers are numpy arrays (the call copies and
    blocks), or contiguous tensors on the scene's device, used in place on `stream` (a torch stream or a raw
    hipStream_t; default: torch's current stream) -- the call then returns without waiting unless stats is asked for.
    Calls on one scene share its workspace: order them on one stream, or synchronise between them.  With camera_rays'
    rays and states, the in-order sum over a pixel's samples equals engine.run's accum bit for bit."""
    handle = _native_scene(objects)
    n, rays_ptr, dev = _rays(rays, handle.device)
    spp = int(spp)
    if spp < 1:
        raise ValueError("spp must be >= 1")
    rng_ptr, rng_dev = (None, None) if rng is None else address(rng, "rng", ("uint64",), shape=(n * spp,), device_index=handle.device,
                                                                tensor_dtypes=("int64", "uint64"))
    if out is None:
        if dev:
            import torch
            out = torch.empty((n, 3), dtype=torch.float64, device=rays.device)
        else:
            out = np.empty((n, 3), np.float64)
    out_ptr, out_dev = address(out, "out", ("float64",), shape=(n, 3), device_index=handle.device)
    same_place(rays=dev, rng=rng_dev, out=out_dev)
    background = scene_background(objects, handle, background)
    q = rt_radiance_params()
    q.flags = (RT_OUT_DEVICE if dev else 0) | (RT_GLOBAL_SCENE if global_scene else 0)
    q.spp, q.max_depth, q.sample_base, q.seed, q.id_base = spp, int(max_depth), int(sample_base), int(seed), int(id_base)
    for c in range(3):
        q.background[c] = float(background[c])
    q.stream = stream_handle(stream, rays.device if dev else None)
    st = rt_stats()
    check(lib.rt_radiance_rays(handle, ctypes.byref(q), ctypes.c_void_p(rays_ptr), None if rng_ptr is None else ctypes.c_void_p(rng_ptr), n,
                               ctypes.c_void_p(out_ptr), ctypes.byref(st) if stats else None), "radiance_rays")
    return (out, {"segments": st.segments, "primary": st.primary, "ms": st.ms}) if stats else out


def camera_rays(cam, width, height, spp, seed=0, sample_base=0, bands=None, device=None, stream=None):
    """rt_camera_rays: the renderer's own camera rays as data.  Returns (rays, rng): entry (ly * width + lx) * spp + j of
    rays ((local_pixels * spp, 7) float64) and rng ((local_pixels * spp,) PCG states) holds the ray engine.run starts at
    local pixel (lx, ly) for sample sample_base + j with `seed`, and the generator state after the camera's draws.
    bands: (band_rows, band_count, band_index), or None for the whole frame.  device None: numpy arrays (uint64 states;
    computed on GPU 0); a device index or torch device: tensors there (int64 states: torch's 64-bit integer type), written
    on `stream` (default: torch's current stream) without waiting.  Needs no scene."""
    if not hasattr(cam, "c"):
        raise TypeError("cam must be an art.camera")
    p = rt_params()
    p.width, p.height, p.spp, p.seed, p.fp_mode = int(width), int(height), int(spp), int(seed), RT_FP64
    p.band_rows, p.band_count, p.band_index = (int(height), 1, 0) if bands is None else (int(b) for b in bands)
    rows = check(lib.rt_local_rows(ctypes.byref(p), None), "rt_local_rows")
    if p.spp < 1:
        raise ValueError("spp must be >= 1")
    ne = rows * p.width * p.spp
    if device is None:
        stream_handle(stream, None)
        rays, rng = np.empty((ne, 7), np.float64), np.empty((ne,), np.uint64)
        rays_ptr, rng_ptr, index = rays.ctypes.data, rng.ctypes.data, 0
    else:
        import torch
        tdev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if tdev.type != "cuda":
            raise ValueError("device must be a GPU (an index or a cuda torch.device), or None for numpy arrays")
        index = tdev.index or 0
        rays = torch.empty((ne, 7), dtype=torch.float64, device=tdev)
        rng = torch.empty((ne,), dtype=torch.int64, device=tdev)
        rays_ptr, rng_ptr = rays.data_ptr(), rng.data_ptr()
        p.flags = RT_OUT_DEVICE
        p.stream = stream_handle(stream, tdev)
    check(lib.rt_camera_rays(ctypes.byref(cam.c), ctypes.byref(p), int(sample_base), index, ctypes.c_void_p(rays_ptr), ctypes.c_void_p(rng_ptr)),
          "camera_rays")
    return rays, rng
