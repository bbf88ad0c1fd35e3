"""rt_radiance_grad without a device: the binding, every refusal (before any device work), the Python wrappers' buffer
checks, the C++ facade, the exact accumulator of grad_fixed.h driven by a stand-alone g++ program against
fractions.Fraction, and the new kernels' register budgets.  Host-only."""
import ctypes
import os
import random
import re
import shutil
import struct
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import RT_GLOBAL_SCENE, RT_OUT_DEVICE, RT_PROFILE, lib, rt_radiance_params, rt_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

RT_OK, RT_E_INVALID, RT_E_DEVICE = 0, -1, -3
N = 5


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def world():
    return art.scene_manager().build("c1")


# ------------------------------------------------------------------------------------------------ the binding
def test_the_header_declares_what_the_bindings_bind():
    header = open(os.path.join(ROOT, "include", "art.h")).read()
    declared = set(re.findall(r"\b(rt_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert "rt_radiance_grad" in declared
    nm = subprocess.run(["nm", "-D", "--defined-only", art._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T rt_radiance_grad" in nm
    assert set(declared) == set(art._lib.SIGNATURES)
    restype, argtypes = art._lib.SIGNATURES["rt_radiance_grad"]
    assert restype is ctypes.c_int and len(argtypes) == 11
    assert argtypes[1] == ctypes.POINTER(rt_radiance_params) and argtypes[5] is ctypes.c_int64 and argtypes[10] == ctypes.POINTER(rt_stats)
    assert re.search(r"#define RT_ABI_VERSION 5\b", header)  # additive
    assert (art.grad.TEXTURE_DOUBLES, art.grad.MATERIAL_DOUBLES) == (4, 5)
    for name in ("radiance_grad", "render_grad", "differentiable_radiance"):
        assert name in art.__all__ and callable(getattr(art, name))


# ------------------------------------------------------------------------------------------------ refusals
def _call(world, n=N, scene=True, params=True, rays=True, weights=True, radiance=True, grads=True, rng=False, stats=False, **fields):
    m = max(1, min(n, 64))  # (a refused call reads nothing)
    r, w, out = np.zeros((m, 7)), np.zeros((m, 3)), np.zeros((m, 3))
    gt, gm, gb = np.zeros((4096, 4)), np.zeros((4096, 5)), np.zeros(3)
    q = rt_radiance_params(max_depth=50)
    for k, v in fields.items():
        setattr(q, k, v)
    states = np.zeros(m * max(1, min(q.spp, 64)), np.uint64) if rng else None
    st = rt_stats()
    g = (_ptr(gt), _ptr(gm), _ptr(gb)) if grads else (None, None, None)
    return lib.rt_radiance_grad(world.objects._native if scene else None, ctypes.byref(q) if params else None, _ptr(r) if rays else None,
                                _ptr(states) if rng else None, _ptr(w) if weights else None, n, _ptr(out) if radiance else None, *g,
                                ctypes.byref(st) if stats else None)


def _refused(world, **kw):
    return _call(world, **kw) == RT_E_INVALID and len(lib.rt_last_error()) > 0


def test_null_arguments_are_refused(world):
    assert _refused(world, scene=False)
    assert _refused(world, params=False)
    assert _refused(world, rays=False)
    assert _refused(world, weights=False)
    assert _refused(world, weights=False, radiance=False, grads=False)  # a refusal comes before "nothing asked for"


@pytest.mark.parametrize("n", [-1, (1 << 30) + 1, 1 << 40])
def test_ray_counts_outside_the_range_are_refused(world, n):
    assert _refused(world, n=n)
    assert b"n must be" in lib.rt_last_error()


def test_more_paths_than_a_call_holds_are_refused_with_the_limit_named(world):
    assert _refused(world, n=1 << 30, spp=3)
    assert b"kMaxPassSlots" in lib.rt_last_error() and b"2^31" in lib.rt_last_error()
    assert _refused(world, n=3, spp=1 << 30)


@pytest.mark.parametrize("flag", [RT_PROFILE, 8, 16, 32, 64, 128, 256, 512, 1024, 1 << 30])
def test_unknown_flag_bits_are_refused(world, flag):
    assert _refused(world, flags=flag)
    assert _refused(world, flags=flag | RT_OUT_DEVICE)


def test_parameters_outside_their_range_are_refused(world):
    assert _refused(world, max_depth=0)
    assert _refused(world, max_depth=-1)
    assert _refused(world, spp=-1)
    assert _refused(world, stream=1234)                      # a stream without RT_OUT_DEVICE
    assert _refused(world, id_base=(1 << 32) - N + 1)        # id_base + n > 2^32
    assert _refused(world, id_base=1 << 63)
    assert _refused(world, id_base=(1 << 64) - 1)            # must not wrap


@pytest.mark.parametrize("fields", [{}, {"flags": RT_OUT_DEVICE}, {"flags": RT_GLOBAL_SCENE, "spp": 8}, {"flags": RT_OUT_DEVICE, "stream": 1234}])
def test_zero_rays_or_no_output_is_ok_and_touches_no_device(world, fields):
    # no device on a host-only machine: RT_OK shows the call returned before any device work
    assert _call(world, n=0, **fields) == RT_OK
    assert _call(world, n=0, rays=False, weights=False, radiance=False, grads=False, stats=True, **fields) == RT_OK
    assert _call(world, radiance=False, grads=False, **fields) == RT_OK
    assert _call(world, radiance=False, grads=False, stats=True, **fields) == RT_OK


@pytest.mark.skipif(lib.rt_device_count() > 0, reason="checks the no-device failure path")
def test_a_valid_call_without_a_device_fails_loudly(world):
    assert _call(world) == RT_E_DEVICE  # the arguments passed every check
    assert _call(world, radiance=False) == RT_E_DEVICE                      # radiance alone may be NULL
    assert _call(world, grads=False) == RT_E_DEVICE                         # and so may the gradients
    assert _call(world, spp=0) == RT_E_DEVICE                               # 0 samples is taken as 1
    assert _call(world, id_base=(1 << 32) - N, spp=4) == RT_E_DEVICE        # the last valid stream id
    assert _call(world, id_base=(1 << 63), rng=True) == RT_E_DEVICE         # id_base is ignored when states are given
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.radiance_grad(world, np.zeros((N, 7)), np.zeros((N, 3)))


# ------------------------------------------------------------------------------------------------ the wrappers
def test_python_wrapper_refuses_wrong_dtypes_shapes_and_strides(world):
    rays, w = np.zeros((N, 7)), np.zeros((N, 3))
    for bad in (rays.astype(np.float32), np.zeros((N, 6)), np.zeros(7 * N), np.zeros((N, 14))[:, ::2], np.zeros((7, N)).T):
        with pytest.raises(ValueError):
            art.radiance_grad(world, bad, w)
    with pytest.raises(TypeError):
        art.radiance_grad(world, rays.tolist(), w)
    for bad in (w.astype(np.float32), np.zeros((N, 4)), np.zeros((N + 1, 3)), np.zeros((N, 6))[:, ::2], np.zeros(3 * N), np.zeros((1, 3))):
        with pytest.raises(ValueError):
            art.radiance_grad(world, rays, bad)
        with pytest.raises(ValueError):
            art.radiance_grad(world, rays, w, out_radiance=bad)
    with pytest.raises(TypeError):
        art.radiance_grad(world, rays, w.tolist())
    for bad in (np.zeros(N, np.int64), np.zeros(N + 1, np.uint64), np.zeros(2 * N, np.uint64)[::2]):
        with pytest.raises(ValueError):
            art.radiance_grad(world, rays, w, rng=bad)
    with pytest.raises(ValueError):
        art.radiance_grad(world, rays, w, spp=3, rng=np.zeros(N, np.uint64))
    with pytest.raises(ValueError):
        art.radiance_grad(world, rays, w, spp=0)
    with pytest.raises(ValueError):
        art.radiance_grad(world, rays, w, stream=1234)  # a stream belongs to device tensors
    with pytest.raises(TypeError):
        art.radiance_grad(art.hittable_list(), rays, w)  # not compiled
    cam = art.camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 16 / 9, 0.0, 5.0)
    with pytest.raises(ValueError):
        art.render_grad(world, cam, 16, 9, 2, np.zeros((9, 16, 4)))
    with pytest.raises(ValueError):
        art.render_grad(world, cam, 16, 9, 2, np.zeros((16, 9, 3)))
    with pytest.raises(TypeError):
        art.render_grad(world, cam, 16, 9, 2, [[0.0]])


def test_python_wrapper_refuses_host_tensors_and_mixed_buffers(world):
    import torch
    rays, w = np.zeros((N, 7)), np.zeros((N, 3))
    with pytest.raises(ValueError):
        art.radiance_grad(world, torch.zeros((N, 7), dtype=torch.float64), w)   # a tensor, but on the host
    with pytest.raises(ValueError):
        art.radiance_grad(world, rays, torch.zeros((N, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        art.radiance_grad(world, rays, w, out_radiance=torch.zeros((N, 3), dtype=torch.float64))


def test_the_cpp_facade_compiles(tmp_path):
    src = tmp_path / "q.cpp"
    src.write_text("""
#include "art_engine.hpp"
int main() {
    art::scene_manager sm("assets");
    art::scene world = sm.build("6");
    const int n = 32;
    std::vector<double> rays(7 * n), w(3 * n, 1.0), radiance(3 * n), gt(4 * 64), gm(5 * 64), gb(3);
    art::radiance_options o;
    o.spp = 4;
    o.background = world.background;
    rt_stats st{};
    art::radiance_grad(world, rays.data(), w.data(), n, radiance.data(), gt.data(), gm.data(), gb.data(), o, nullptr, &st);
    art::radiance_grad(world, rays.data(), w.data(), n, nullptr, nullptr, nullptr, gb.data());
    return st.segments >= st.primary ? 0 : 1;
}
""")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


# ------------------------------------------------------------------------------------------------ the exact accumulator
FRAC = 96  # grad_fixed.h: the quantum is 2^-96


def _hex(x):
    return struct.pack(">d", x).hex()


def _unhex(s):
    return struct.unpack(">d", bytes.fromhex(s))[0]


def _quanta(x):
    """trunc(x * 2^96) as a Python integer: the magnitude truncated towards zero."""
    f = Fraction(x) * (1 << FRAC)
    q = abs(f.numerator) // f.denominator
    return -q if f < 0 else q


@pytest.fixture(scope="module")
def fixed(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("grad_fixed") / "grad_fixed_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "another_raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "grad_fixed_check.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, check=True)
        return out.stdout.split("\n")[:len(lines)]
    return run


def _random_doubles(rnd, n, whole_quanta):
    """n doubles with magnitudes spanning 2^-60 .. 2^40 and mixed signs; whole_quanta: multiples of 2^-96 only."""
    out = []
    for _ in range(n):
        e = rnd.randint(-60, 39)
        bits = min(52, e + FRAC) if whole_quanta else 52
        m = (1 << bits) + rnd.getrandbits(bits)
        x = float(Fraction(m, 1 << bits) * Fraction(2) ** e)
        out.append(-x if rnd.random() < 0.5 else x)
    return out


@pytest.mark.parametrize("whole_quanta", [True, False])
def test_sums_in_every_order_are_the_correctly_rounded_exact_sum(fixed, whole_quanta):
    rnd = random.Random(20 + whole_quanta)
    xs = _random_doubles(rnd, 10000, whole_quanta)
    assert min(abs(x) for x in xs) < 2.0 ** -55 and max(abs(x) for x in xs) > 2.0 ** 35
    if whole_quanta:  # nothing is truncated: the sum of the doubles themselves
        exact = sum(Fraction(x) for x in xs)
        assert all(Fraction(_quanta(x), 1 << FRAC) == Fraction(x) for x in xs)
    else:             # full mantissas: each term truncated to whole quanta first, as documented
        exact = Fraction(sum(_quanta(x) for x in xs), 1 << FRAC)
        assert any(Fraction(_quanta(x), 1 << FRAC) != Fraction(x) for x in xs)
    want = _hex(float(exact))  # int / int true division rounds correctly
    orders = [xs, xs[::-1], sorted(xs), sorted(xs, key=abs), sorted(xs, key=abs, reverse=True)]
    for _ in range(3):
        shuffled = list(xs)
        rnd.shuffle(shuffled)
        orders.append(shuffled)
    got = fixed(["S " + " ".join(_hex(x) for x in order) for order in orders])
    assert got == [want] * len(orders)
    # a float sum of the same terms does depend on the order: the property is not vacuous
    assert len({sum(order) for order in orders}) > 1


def test_rounding_is_to_nearest_even_and_cancellation_is_exact(fixed):
    one, ulp = 1.0, 2.0 ** -52
    cases = [
        ([one, ulp / 2], one),                       # a tie: to even (down)
        ([one + ulp, ulp / 2], one + 2 * ulp),       # a tie: to even (up)
        ([one, ulp / 2, 2.0 ** -96], one + ulp),     # above the tie by one quantum
        ([one, -ulp / 4], one),                      # below 1: the spacing is ulp / 2, this is a tie to even
        ([2.0 ** 40, 2.0 ** -60, -(2.0 ** 40)], 2.0 ** -60),
        ([2.0 ** 53, 1.0, 1.0], 2.0 ** 53 + 2),
        ([3.5, -3.5], 0.0),
        ([-1.0, -ulp / 2, -(2.0 ** -96)], -(one + ulp)),
        ([(2.0 ** 53 - 1) * 2.0 ** 2, (2.0 ** 53 - 1) * 2.0 ** 2], (2.0 ** 53 - 1) * 2.0 ** 3),
    ]
    got = fixed(["S " + " ".join(_hex(x) for x in xs) for xs, _ in cases])
    assert got == [_hex(want) for _, want in cases]
    assert got[6] == "0" * 16  # +0.0


def test_truncation_and_refusal_are_as_documented(fixed):
    q = 2.0 ** -FRAC

    def limbs(v):
        v &= (1 << 192) - 1
        return "ok %016x %016x %016x" % (v >> 128, (v >> 64) & (2 ** 64 - 1), v & (2 ** 64 - 1))
    cases = [(0.0, limbs(0)), (-0.0, limbs(0)), (q, limbs(1)), (-q, limbs(-1)), (q / 2, limbs(0)), (-q / 2, limbs(0)),
             (1.75 * q, limbs(1)), (-1.75 * q, limbs(-1)),           # towards zero, both signs
             (5e-324, limbs(0)), (2.0 ** -1022, limbs(0)),           # subnormals and tiny normals
             (1.0, limbs(1 << 96)), (-1.0, limbs(-(1 << 96))), (2.0 ** -32, limbs(1 << 64)), (2.0 ** 32, limbs(1 << 128)),
             (1.0 + 2.0 ** -52, limbs((1 << 96) + (1 << 44))),
             (2.0 ** 56 - 2.0 ** 3, limbs((1 << 152) - (1 << 99))),  # the largest magnitude an accumulator takes
             (2.0 ** 56, "refused"), (-(2.0 ** 56), "refused"), (1e300, "refused"),
             (float("inf"), "refused"), (float("-inf"), "refused"), (float("nan"), "refused")]
    assert fixed(["C " + _hex(x) for x, _ in cases]) == [want for _, want in cases]
    for x, want in cases:
        if want != "refused":
            assert limbs(_quanta(x)) == want  # the test's own model agrees
    # a refused term turns the sum to NaN, wherever it stands
    assert fixed(["S " + " ".join(_hex(x) for x in (1.0, float("inf"), 2.0)), "S " + _hex(2.0 ** 56), "S " + _hex(1.0)]) == ["nan", "nan", _hex(1.0)]


# ------------------------------------------------------------------------------------------------ the kernels
def test_the_new_kernels_are_in_the_library_and_meet_their_register_budgets():
    ks = kernel_resources.kernels(os.path.join(ROOT, "another_raytracer_amd", "libart.so"))
    grad = {n: k for n, k in ks.items() if "k_radiance_grad" in n}
    # the three HBM-scene feature sets with solid / checker or all textures, the two with triangles also with barycentric images
    assert len(grad) == 8, sorted(grad)
    for n, k in grad.items():
        # three waves per SIMD: 512 / 3 = 168 VGPRs (AGPRs included), 256-lane blocks, no static LDS
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 168 and k[".max_flat_workgroup_size"] == 256, (n, k)
        assert k[".group_segment_fixed_size"] == 0, (n, k)
    found = [k for n, k in ks.items() if "k_grad_finish" in n]
    assert len(found) == 1 and found[0][".vgpr_count"] + found[0].get(".agpr_count", 0) <= 168 and found[0].get(".vgpr_spill_count", 0) == 0
