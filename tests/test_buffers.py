"""another_raytracer_amd/_buffers.py -- what every entry point accepts as a caller's buffer -- as a table over the module:
numpy arrays and CPU tensors directly, device tensors through a stand-in with a tensor's data_ptr / device / dtype /
is_contiguous / shape (no GPU is touched)."""
import types

import numpy as np
import pytest
import torch

from another_raytracer_amd import _buffers as B

F64, U8 = ("float64",), ("uint8",)


class FakeTensor:
    """A contiguous-or-not tensor of `dtype` and `shape` at address 0x1000 on cuda:`index` (or the CPU)."""

    def __init__(self, shape, dtype="torch.float64", index=0, contiguous=True, itemsize=8, cpu=False):
        self.shape, self.dtype, self._contiguous, self._itemsize = tuple(shape), dtype, contiguous, itemsize
        self.device = types.SimpleNamespace(type="cpu" if cpu else "cuda", index=None if cpu else index)

    def data_ptr(self):
        return 0x1000

    def is_contiguous(self):
        return self._contiguous

    def element_size(self):
        return self._itemsize


def test_is_tensor():
    assert B.is_tensor(torch.zeros(1)) and B.is_tensor(FakeTensor((1,)))
    assert not B.is_tensor(np.zeros(1)) and not B.is_tensor([0.0]) and not B.is_tensor(None)


# (buffer, address()'s keyword arguments) -> (is_device,) or the exception class
ACCEPTED = [
    # the exact-shape rule (query_rays, radiance_rays, render_views, update_triangles)
    (np.zeros((5, 7)), dict(dtypes=F64, shape=(5, 7), device_index=0), False),
    (np.zeros((0, 7)), dict(dtypes=F64, shape=(0, 7), device_index=0), False),
    (np.zeros(5, np.bool_), dict(dtypes=("uint8", "bool"), shape=(5,), device_index=0), False),
    (FakeTensor((5, 7)), dict(dtypes=F64, shape=(5, 7), device_index=0), True),
    (FakeTensor((5, 7), index=None), dict(dtypes=F64, shape=(5, 7), device_index=0), True),  # "cuda" is cuda:0
    (FakeTensor((5, 7), index=3), dict(dtypes=F64, shape=(5, 7), device_index=3), True),
    (FakeTensor((5,), "torch.int64"), dict(dtypes=("uint64",), tensor_dtypes=("int64", "uint64"), shape=(5,), device_index=0), True),
    (FakeTensor((5,), "torch.bool", itemsize=1), dict(dtypes=("uint8", "bool"), shape=(5,), device_index=0), True),
    # the "at least" rules (engine.run and its kin): elements or bytes, CPU tensors are host buffers, a device tensor anywhere
    (np.zeros((4, 3)), dict(dtypes=F64, at_least=12), False),
    (np.zeros((5, 3)), dict(dtypes=F64, at_least=12), False),
    (np.zeros(12, np.uint8), dict(dtypes=U8, min_bytes=12), False),
    (np.zeros(3, np.float32), dict(dtypes=B.ANY, min_bytes=12), False),
    (torch.zeros((4, 3), dtype=torch.float64), dict(dtypes=F64, at_least=12, tensor_dtypes=8), False),
    (torch.zeros(12, dtype=torch.int64), dict(dtypes=F64, at_least=12, tensor_dtypes=8), False),    # 8-byte elements
    (torch.zeros(3, dtype=torch.float32), dict(dtypes=U8, min_bytes=12, tensor_dtypes=B.ANY), False),  # raw bytes
    (torch.zeros(12, dtype=torch.int32), dict(dtypes=("int32",), at_least=12), False),
    (FakeTensor((4, 3), index=5), dict(dtypes=F64, at_least=12, tensor_dtypes=8), True),
]
REFUSED = [
    # wrong dtype
    (np.zeros((5, 7), np.float32), dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    (np.zeros(5, np.int64), dict(dtypes=("uint64",), tensor_dtypes=("int64", "uint64"), shape=(5,), device_index=0), ValueError),
    (FakeTensor((5, 7), "torch.float32", itemsize=4), dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    (FakeTensor((5,), "torch.float64"), dict(dtypes=("uint64",), tensor_dtypes=("int64", "uint64"), shape=(5,), device_index=0), ValueError),
    (np.zeros(12, np.int8), dict(dtypes=U8, min_bytes=12, tensor_dtypes=B.ANY), ValueError),
    (torch.zeros(24, dtype=torch.float32), dict(dtypes=F64, at_least=12, tensor_dtypes=8), ValueError),
    (torch.zeros(12, dtype=torch.int64), dict(dtypes=("int32",), at_least=12), ValueError),
    # non-contiguous
    (np.zeros((5, 14))[:, ::2], dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    (np.zeros((7, 5)).T, dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    (FakeTensor((5, 7), contiguous=False), dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    (torch.zeros((4, 6), dtype=torch.float64)[:, ::2], dict(dtypes=F64, at_least=12, tensor_dtypes=8), ValueError),
    (np.zeros(24, np.uint8)[::2], dict(dtypes=U8, min_bytes=12), ValueError),
    # wrong shape under the exact rule: more, fewer, another rank with the same elements
    (np.zeros((6, 7)), dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    (np.zeros((4, 7)), dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    (np.zeros(35), dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    (FakeTensor((5, 8)), dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    # too small under the "at least" rules
    (np.zeros(11), dict(dtypes=F64, at_least=12), ValueError),
    (np.zeros(11, np.uint8), dict(dtypes=U8, min_bytes=12), ValueError),
    (torch.zeros(11, dtype=torch.float64), dict(dtypes=F64, at_least=12, tensor_dtypes=8), ValueError),
    (torch.zeros(2, dtype=torch.float32), dict(dtypes=U8, min_bytes=12, tensor_dtypes=B.ANY), ValueError),
    (FakeTensor((11,)), dict(dtypes=F64, at_least=12, tensor_dtypes=8), ValueError),
    # wrong device index, and a CPU tensor where the scene's device is asked for
    (FakeTensor((5, 7), index=1), dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    (FakeTensor((5, 7), index=0), dict(dtypes=F64, shape=(5, 7), device_index=2), ValueError),
    (FakeTensor((5, 7), cpu=True), dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    (torch.zeros((5, 7), dtype=torch.float64), dict(dtypes=F64, shape=(5, 7), device_index=0), ValueError),
    # neither an array nor a tensor
    ([0.0] * 35, dict(dtypes=F64, shape=(5, 7), device_index=0), TypeError),
    (None, dict(dtypes=F64, at_least=1), TypeError),
    (bytearray(12), dict(dtypes=U8, min_bytes=12), TypeError),
]


@pytest.mark.parametrize("case", range(len(ACCEPTED)))
def test_address_accepts(case):
    buf, kw, is_device = ACCEPTED[case]
    addr, dev = B.address(buf, "buf", **kw)
    assert dev is is_device
    assert addr == (buf.ctypes.data if isinstance(buf, np.ndarray) else buf.data_ptr())


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_address_refuses(case):
    buf, kw, exc = REFUSED[case]
    with pytest.raises(exc) as e:
        B.address(buf, "the_argument", **kw)
    assert "the_argument" in str(e.value)  # the message names the argument ...
    if exc is ValueError and "shape" in kw and "live on" not in str(e.value):
        assert str(tuple(kw["shape"])) in str(e.value)  # ... and the requirement


def test_same_place():
    assert B.same_place(rays=False, t_max=False, out=False) is False
    assert B.same_place(rays=True, t_max=None, out=True) is True
    assert B.same_place(out=False, accum=None) is False
    for mixed in (dict(rays=True, out=False), dict(rays=False, t_max=True, out=False), dict(out=False, accum=True)):
        with pytest.raises(ValueError) as e:
            B.same_place(**mixed)
        assert all(name in str(e.value) for name in mixed)


def test_stream_handle(monkeypatch):
    # host buffers take no stream
    assert B.stream_handle(None, None) is None
    with pytest.raises(ValueError, match="stream applies to device tensors only"):
        B.stream_handle(1234, None)
    drained = []
    default = types.SimpleNamespace(cuda_stream=0, synchronize=lambda: drained.append("default"))
    side = types.SimpleNamespace(cuda_stream=0x5150, synchronize=lambda: drained.append("side"))
    monkeypatch.setattr(torch.cuda, "default_stream", lambda device=None: default)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: side)
    # a side stream, as a torch stream, as a raw handle and as torch's current stream: passed on, nothing waited for
    assert B.stream_handle(side, "cuda:0") == 0x5150
    assert B.stream_handle(0x77, "cuda:0") == 0x77
    assert B.stream_handle(None, "cuda:0") == 0x5150
    assert drained == []
    # the null handle (torch's default stream, a raw 0, or the current stream being the default one): the library runs on
    # its own stream and waits, so the default stream is drained first
    assert not B.stream_handle(default, "cuda:0") and drained == ["default"]
    assert not B.stream_handle(0, "cuda:0") and drained == ["default"] * 2
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: default)
    assert not B.stream_handle(None, "cuda:0") and drained == ["default"] * 3


def test_scene_background():
    import another_raytracer_amd as art
    world = art.scene_manager().build("1")
    assert B.scene_background(world, None, (1.0, 2.0, 3.0)) == (1.0, 2.0, 3.0)     # the caller's wins
    assert tuple(B.scene_background(world, None)) == tuple(world.background)       # a scene_manager scene: its own
    from another_raytracer_amd.rays import _native_scene
    handle = _native_scene(world.objects)                                          # a bare handle: what the compiled scene records
    assert tuple(B.scene_background(world.objects, handle)) == tuple(float(x) for x in world.background)
