"""A caller's buffer, as every entry point of the package takes one: a C-contiguous numpy array (the host path: the
library copies and blocks) or a contiguous torch tensor (on a device: used in place; on the CPU, where the entry point
allows it: a host buffer like a numpy array).  address() checks one buffer and returns where it is, same_place() that a
call's buffers agree on it, stream_handle() the stream a device call runs on; scene_background() is the one default the
calls on a compiled scene share."""
import ctypes
import math

import numpy as np

from ._lib import check, lib, rt_scene_info
from .scene import scene

ANY = "any"  # dtypes: any element type


def is_tensor(x):
    return hasattr(x, "data_ptr")


def _requirement(tensor, dtypes, shape, at_least, min_bytes):
    """The words of a refusal: dtypes is a tuple of dtype names ("float64"), an element size in bytes, or ANY."""
    what = "" if dtypes is ANY else f"{dtypes}-byte " if isinstance(dtypes, int) else " or ".join(dtypes) + " "
    size = f"shape {tuple(shape)}" if shape is not None else f">= {at_least} elements" if at_least is not None else f">= {min_bytes} bytes"
    return f"a contiguous {what}tensor of {size}" if tensor else f"a C-contiguous {what}array of {size}"


def address(buf, what, dtypes, shape=None, at_least=None, min_bytes=None, device_index=None, tensor_dtypes=None):
    """(address, is_device) of the buffer `what`: a numpy array of `dtypes`, or a tensor of tensor_dtypes (default: the
    same), contiguous, and of exactly `shape`, or of at least `at_least` elements or `min_bytes` bytes.  device_index: the
    scene's device, on which a tensor must then live (a CPU tensor is refused); None: a tensor on any device, and a CPU
    tensor is a host buffer.  TypeError for anything but an array or a tensor, ValueError for one that does not fit.
    engine.run passes through here per frame: nothing is formatted unless the buffer is refused."""
    tensor = not isinstance(buf, np.ndarray)
    if tensor:
        if not hasattr(buf, "data_ptr"):
            raise TypeError(f"{what} must be a numpy array or a torch tensor")
        if tensor_dtypes is not None:
            dtypes = tensor_dtypes
        itemsize, ok = buf.element_size(), buf.is_contiguous()
    else:
        itemsize, ok = buf.dtype.itemsize, buf.flags.c_contiguous
    if isinstance(dtypes, int):
        ok = ok and itemsize == dtypes
    elif dtypes is not ANY:
        ok = ok and (str(buf.dtype)[6:] in dtypes if tensor else any(buf.dtype == d for d in dtypes))  # "torch.float64"[6:]
    if shape is not None:
        ok = ok and tuple(buf.shape) == tuple(shape)
    elif at_least is not None:
        ok = ok and math.prod(buf.shape) >= at_least
    else:
        ok = ok and math.prod(buf.shape) * itemsize >= min_bytes
    if not ok:
        raise ValueError(f"{what} must be {_requirement(tensor, dtypes, shape, at_least, min_bytes)}")
    if not tensor:
        return buf.ctypes.data, False
    device = buf.device
    if device_index is not None and (device.type == "cpu" or (device.index or 0) != device_index):
        raise ValueError(f"{what} must live on the scene's device (cuda:{device_index})")
    return buf.data_ptr(), device.type != "cpu"


def same_place(**places):
    """Whether the call's buffers live on the device, given name=is_device for each (None: a buffer that was not passed);
    ValueError unless they all live on the host or all on the device."""
    where = places.values()
    if True in where and False in where:
        raise ValueError(" and ".join(k for k, v in places.items() if v is not None) + " must all live on the host (numpy arrays) or all on "
                         "the device (tensors)")
    return True in where


def stream_handle(stream, device):
    """The raw hipStream_t a call on tensors of `device` runs on: `stream` (a torch stream or a handle; None: torch's
    current stream there).  The null handle means "the library's own stream, and wait": torch's default stream is then
    drained first, so the inputs are complete when the call is made (the library's stream is not ordered after it).
    device None -- host buffers -- takes no stream: the host path runs on the scene's own stream and blocks."""
    if device is None:
        if stream is not None:
            raise ValueError("stream applies to device tensors only: the host path runs on the scene's own stream and blocks")
        return None
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(device)
    handle = getattr(stream, "cuda_stream", stream)
    if not handle:
        torch.cuda.default_stream(device).synchronize()
    return handle


def scene_background(world, handle, background=None):
    """The background a call on a compiled scene renders against: the caller's, else the scene_manager scene's own, else
    what the compiled scene records (rt_scene_info_get)."""
    if background is None and isinstance(world, scene):
        background = world.background
    if background is None:
        info = rt_scene_info()
        check(lib.rt_scene_info_get(handle, ctypes.byref(info)), "rt_scene_info_get")
        background = tuple(info.background)
    return background
