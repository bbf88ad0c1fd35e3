"""The two calls every kind of scene update is made of (rt_scene_update_* and rt_scene_*_get, include/art.h), as deform.py
and appearance.py wrap them per kind."""
import ctypes

import numpy as np

from ._lib import RT_OUT_DEVICE, check, lib, rt_update_params
from ._buffers import address, stream_handle
from .rays import _native_scene


def get(world, name, *shapes):
    """The count-then-fill getter rt_<name>_get: one (n, ...) array per out pointer, given as (trailing shape, dtype)."""
    fn = getattr(lib, f"rt_{name}_get")
    handle = _native_scene(world)
    none = (None,) * len(shapes)
    n = check(fn(handle, *none, 0), name)
    outs = tuple(np.empty((n, *shape), dtype) for shape, dtype in shapes)
    if n:
        check(fn(handle, *(ctypes.c_void_p(o.ctypes.data) for o in outs), n), name)
    return outs


def update(world, v, arg, shapes, rule, name, first, stream, timing, dtypes=("float64",), lead=()):
    """rt_scene_<name>: v (the caller's argument `arg`) holds records [first, first + n); its shape is (n, *one of shapes),
    which `rule` says in words.  dtypes: the element type (update_texels: uint8); lead: the arguments the C function takes
    between its params and its buffer (update_texels: the image)."""
    handle = _native_scene(world)
    if not hasattr(v, "shape"):
        raise TypeError(f"{arg} must be a numpy array or a torch tensor")
    shape = tuple(int(x) for x in v.shape)
    if shape[1:] not in shapes:
        raise ValueError(f"{arg} must have {rule}")
    ptr, dev = address(v, arg, dtypes, shape=shape, device_index=handle.device)
    u = rt_update_params()
    u.flags = RT_OUT_DEVICE if dev else 0
    u.stream = stream_handle(stream, v.device if dev else None)
    ms = ctypes.c_double()
    check(getattr(lib, f"rt_scene_{name}")(handle, ctypes.byref(u), *lead, ctypes.c_void_p(ptr), int(first), shape[0], ctypes.byref(ms) if timing else None), name)
    return ms.value if timing else None
