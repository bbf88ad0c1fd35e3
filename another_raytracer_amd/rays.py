"""Ray queries on a compiled scene (rt_query_rays, include/art.h): hittable_list::hit(r, 0.001, t_max, rec) for arbitrary
rays through the renderer's own BVH traversal -- the closest hit with the whole hit_record, or any-hit occlusion.

    world = art.scene_manager().build("cow")
    hits = art.query_rays(world.objects, rays)                       # (n, 12) records; hits.t, hits.point, hits.prim ...
    blocked = art.query_rays(world.objects, shadow_rays, t_max=dist, any_hit=True)   # (n,) uint8

Buffers are numpy arrays (host path: the call copies and blocks) or contiguous float64 torch tensors on the scene's device
(used in place, on torch's current stream, without waiting: the result tensor is ordered after the query on that stream
like any torch operation).
"""
import ctypes

import numpy as np

from ._lib import RT_GLOBAL_SCENE, RT_HIT_DOUBLES, RT_OUT_DEVICE, RT_Q_ANY_HIT, RT_Q_NO_MEDIA, check, lib, rt_query_params
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


def _is_tensor(x):
    return hasattr(x, "data_ptr")


def _f64_buffer(buf, shape, what, dev, device_index):
    """Address of a float64 buffer of exactly `shape`, checked as engine._f64_pointer checks (dtype, contiguity, size) and
    for living where the rays do."""
    if isinstance(buf, np.ndarray):
        if dev:
            raise ValueError(f"{what} must be a torch tensor on the scene's device, as rays is")
        if buf.dtype != np.float64 or not buf.flags.c_contiguous or tuple(buf.shape) != shape:
            raise ValueError(f"{what} must be a C-contiguous float64 array of shape {shape}")
        return buf.ctypes.data
    if _is_tensor(buf):
        if not dev:
            raise ValueError(f"{what} must be a numpy array, as rays is")
        if str(buf.dtype) != "torch.float64" or not buf.is_contiguous() or tuple(buf.shape) != shape:
            raise ValueError(f"{what} must be a contiguous float64 tensor of shape {shape}")
        if buf.device.type == "cpu" or (buf.device.index or 0) != device_index:
            raise ValueError(f"{what} must live on the scene's device (cuda:{device_index})")
        return buf.data_ptr()
    raise TypeError(f"{what} must be a numpy array or a torch tensor")


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
    dev = _is_tensor(rays)
    if not dev and not isinstance(rays, np.ndarray):
        raise TypeError("rays must be a numpy array or a torch tensor")
    if len(rays.shape) != 2 or int(rays.shape[1]) != 7:
        raise ValueError("rays must have shape (n, 7): origin, direction, time")
    n = int(rays.shape[0])
    rays_ptr = _f64_buffer(rays, (n, 7), "rays", dev, handle.device)
    tmax_ptr = None if t_max is None else _f64_buffer(t_max, (n,), "t_max", dev, handle.device)
    if dev:
        import torch
    if any_hit:
        if out is None:
            out = torch.empty((n,), dtype=torch.uint8, device=rays.device) if dev else np.empty((n,), np.uint8)
        elif isinstance(out, np.ndarray):
            if dev or out.dtype not in (np.uint8, np.bool_) or not out.flags.c_contiguous or out.shape != (n,):
                raise ValueError(f"out must be a C-contiguous uint8 or bool array of shape ({n},) living where rays does")
        elif _is_tensor(out):
            if (not dev or str(out.dtype) not in ("torch.uint8", "torch.bool") or not out.is_contiguous() or tuple(out.shape) != (n,)
                    or out.device != rays.device):
                raise ValueError(f"out must be a contiguous uint8 or bool tensor of shape ({n},) on the rays' device")
        else:
            raise TypeError("out must be a numpy array or a torch tensor")
        out_ptr = out.data_ptr() if dev else out.ctypes.data
    else:
        if out is None:
            out = (torch.empty((n, RT_HIT_DOUBLES), dtype=torch.float64, device=rays.device) if dev
                   else np.empty((n, RT_HIT_DOUBLES), np.float64))
        out_ptr = _f64_buffer(out, (n, RT_HIT_DOUBLES), "out", dev, handle.device)
    q = rt_query_params()
    q.flags = ((RT_OUT_DEVICE if dev else 0) | (RT_GLOBAL_SCENE if global_scene else 0) | (RT_Q_ANY_HIT if any_hit else 0)
               | (RT_Q_NO_MEDIA if no_media else 0))
    if dev:
        if stream is None:
            stream = torch.cuda.current_stream(rays.device)
        q.stream = getattr(stream, "cuda_stream", stream)
        if not q.stream:
            # torch's default stream has the null handle, which rt_query_rays reads as "the scene's own stream" (and then
            # waits for the query): that stream is not ordered after the default one, so the inputs are finished first
            torch.cuda.default_stream(rays.device).synchronize()
    elif stream is not None:
        raise ValueError("stream applies to device tensors only: the host path runs on the scene's own stream and blocks")
    hits_arg = None if any_hit else ctypes.c_void_p(out_ptr)
    occ_arg = ctypes.c_void_p(out_ptr) if any_hit else None
    check(lib.rt_query_rays(handle, ctypes.byref(q), ctypes.c_void_p(rays_ptr), None if tmax_ptr is None else ctypes.c_void_p(tmax_ptr),
                            n, hits_arg, occ_arg), "query_rays")
    return out if any_hit else HitRecords(out)
