"""Every compile-time knob that survives in the kernel sources (another_raytracer_amd/csrc) still compiles for gfx950
with a non-default value, device code only (no GPU needed): the diagnostic builds (ART_STATS divergence counters,
ART_TRACE path dumps: the one-object build, kernels_unity.hip), the k_paths leaf test with the per-slot code
(ART_LDS_LEAF_NOREF=0) and the tuning parameters DESIGN.md §4 measured (suspend threshold, waves per SIMD, ring size,
LDS node capacity, k_extend occupancy, k_paths_g's LDS camera-ray ring for A/B).  Dropped experiments are deleted from the sources, not compiled out, so no
other switch exists to rot."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "another_raytracer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# knob sets (source file, flags), each compiled once (sets combine knobs that do not interact, to keep the CPU suite short)
VARIANTS = {
    "stats": ("kernels_unity.hip", ["-DART_STATS", "-DART_SUSPEND_LANES=0", "-DART_POOL_RING=128", "-DART_LDS_NODE_CAP=320"]),
    "trace": ("kernels_unity.hip", ["-DART_TRACE", "-DART_PATHS_G_WAVES=2", "-DART_EXTEND_MIN_WAVES=2", "-DART_LDS_LEAF_NOREF=1"]),
    "paths_ref": ("k_paths.hip", ["-DART_LDS_LEAF_NOREF=0", "-DART_SUSPEND_LANES=16"]),
    "no_ring": ("kernels.hip", ["-DART_LDS_RING_G=0"]),
}
SURVIVING = {"ART_STATS", "ART_TRACE", "ART_LDS_LEAF_NOREF", "ART_SUSPEND_LANES", "ART_PATHS_G_WAVES",
             "ART_POOL_RING", "ART_LDS_NODE_CAP", "ART_EXTEND_MIN_WAVES", "ART_LDS_BLOCK", "ART_LDS_RING_G"}


def _compile(variant, out):
    src, args = variant
    cmd = [HIPCC, "-std=c++17", "-O1", "--offload-arch=gfx950", "--cuda-device-only", "-ffp-contract=off", "-w", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, *args, "-c", os.path.join(CSRC, src), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=1200)


def test_no_other_compile_time_switch_exists():
    # the knobs the sources test with #if / #ifdef / #ifndef are exactly the surviving set (plus include guards)
    found = set()
    for f in os.listdir(CSRC):
        if f.endswith((".h", ".hip", ".cpp")):
            for m in re.finditer(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b[^\n]*", open(os.path.join(CSRC, f)).read(), re.M):
                found |= set(re.findall(r"\bART_[A-Z0-9_]+", m.group(0)))
    assert found <= SURVIVING, sorted(found - SURVIVING)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not in this image")
def test_non_default_knobs_compile_for_gfx950(tmp_path):
    with ThreadPoolExecutor(max_workers=len(VARIANTS)) as ex:
        res = dict(zip(VARIANTS, ex.map(lambda kv: _compile(kv[1], str(tmp_path / (kv[0] + ".o"))), VARIANTS.items())))
    for name, r in res.items():
        assert r.returncode == 0, (name, r.stderr[-2000:])
        assert os.path.getsize(tmp_path / (name + ".o")) > 0
