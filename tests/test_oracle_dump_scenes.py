"""The oracle reads scenes it did not build (oracle/restate.cpp: a scene argument that starts with '{' is a canonical
dump), checked on the CPU before any GPU is involved:

* the twelve builtin scenes through the product's builder, its dump and the oracle's loader equal the oracle's own
  scenes: the dump byte for byte, a render in rgb / acc / segments, closest hits in bits;
* every malformed dump is refused with a message; tests/native/dump_loader_check.cpp repeats that, with every
  truncation of three dumps, as a plain executable under AddressSanitizer and UBSan;
* the recipe scenes of tests/recipes.py (the GPU parity cases of tests/test_gpu_recipe_parity.py) are not trivial: camera
  rays hit geometry, paths bounce, and every primitive and material kind a recipe declares is what some camera ray hits
  first;
* coverage closure: every k_paths_g<F, TF, LM> kernel in libart.so is claimed by a GPU parity case or listed, with its
  reason, in NOT_COMPARED."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd.scene import scene_dump
from tests import recipes
from tests.oracle_lib import ASSETS, oracle, oracle_dump, oracle_probe, oracle_register_image, oracle_render, oracle_render_adaptive, \
    oracle_render_images, oracle_trace_rays
from tests.update_common import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["c1", "1", "2", "3", "4", "5", "6", "7", "8", "cow", "dino", "9"]
IMAGES = {"4": "earthmap.jpg", "8": "earthmap.jpg", "9": os.path.join("models", "capsule", "capsule.jpg")}


# ------------------------------------------------------------------------------------------------ the twelve builtins
@pytest.fixture(scope="module")
def builtin():
    """scene -> (the product's scene, its dump): built once, shared."""
    out = {}
    for s in SCENES:
        if s in IMAGES:
            oracle_register_image(art.imageio.load_image(os.path.join(ASSETS, IMAGES[s])))
        world = art.scene_manager().build(s)
        out[s] = (world, scene_dump(world))
    return out


@pytest.mark.parametrize("scene", SCENES)
def test_builder_dump_loads_into_the_oracles_own_scene(builtin, scene):
    assert oracle_dump(builtin[scene][1]) == oracle_dump(scene)


@pytest.mark.parametrize("scene", SCENES)
def test_dump_renders_like_the_named_scene(builtin, scene):
    a, b = oracle_render(builtin[scene][1], 24, 14, 2), oracle_render(scene, 24, 14, 2)
    assert np.array_equal(a["rgb"], b["rgb"]) and np.array_equal(bits(a["acc"]), bits(b["acc"])) and a["segments"] == b["segments"]


@pytest.mark.parametrize("scene", SCENES)
def test_dump_traces_like_the_named_scene(builtin, scene):
    rays = recipes.pixel_centre_rays(builtin[scene][0], 16, 16)
    assert len(rays) == 256
    ta, na = oracle_trace_rays(builtin[scene][1], rays)
    tb, nb = oracle_trace_rays(scene, rays)
    assert np.isfinite(tb).any()
    assert np.array_equal(bits(ta), bits(tb)) and np.array_equal(bits(na), bits(nb))


# ------------------------------------------------------------------------------------------------ refusals
def _replaced(text, old, new):
    assert text.count(old) >= 1, old
    return text.replace(old, new, 1)


def test_malformed_dumps_are_refused_with_a_message():
    smoke, final = oracle_dump("7"), oracle_dump("1")  # final: the benchmark scene, one bvh of spheres
    cases = {
        "truncated": (smoke[:len(smoke) // 2], "truncated"),
        "truncated in a string": (smoke[:smoke.index('"type":"yz_rect"') + 10], "truncated"),
        "truncated before the end": (smoke.rstrip()[:-1], "truncated"),
        "unknown object type": (_replaced(smoke, '"type":"translate"', '"type":"scale"'), 'unknown object type "scale"'),
        "unknown material type": (_replaced(smoke, '"type":"diffuse_light"', '"type":"neon"'), 'unknown material type "neon"'),
        "unknown texture type": (_replaced(smoke, '"type":"solid"', '"type":"marble"'), 'unknown texture type "marble"'),
        "missing key": (_replaced(smoke, '"k":555,', ""), 'missing key "k"'),
        "missing header key": (_replaced(smoke, '"aperture":0,', ""), 'missing key "aperture"'),
        "short vector": (_replaced(smoke, '"offset":[265,0,295]', '"offset":[265,0]'), "wrong array length"),
        "long vector": (_replaced(smoke, '"offset":[265,0,295]', '"offset":[265,0,295,1]'), "wrong array length"),
        "five box sides": (_replaced(smoke, '"sides":[{"type":"xy_rect","a0":0,"a1":165,"b0":0,"b1":330,"k":165,"mat":{"type":"lambertian","tex":{"type":"solid","c":[0.72999999999999998,0.72999999999999998,0.72999999999999998]}}},', '"sides":['), "wrong array length"),
        "trailing garbage": (smoke.rstrip() + " ]", "trailing garbage"),
        "nesting": ('{"lookfrom":[0,0,0],"lookat":[0,0,1],"vfov":40,"aperture":0,"background":[0,0,0],"objects":[' + '{"type":"list","items":[' * 500 + "]}" * 500 + "]}", "nesting deeper"),
        "box sides": (_replaced(smoke, '"max":[165,165,165]', '"max":[165,166,165]'), "box sides disagree"),
        "bvh nodes": (_replaced(final, '"type":"bvh","nodes":', '"type":"bvh","nodes":1'), "bvh node count"),
        "bvh box": (_replaced(final, '"box":[[-1000,', '"box":[[-1001,'), "bvh box"),
        "unregistered image": ('{"lookfrom":[0,0,0],"lookat":[0,0,1],"vfov":40,"aperture":0,"background":[0,0,0],"objects":[{"type":"sphere","center":[0,0,3],"radius":1,"mat":{"type":"lambertian","tex":{"type":"image","w":7,"h":5,"bpp":3,"fnv1a":"0123456789abcdef"}}}]}', "0123456789abcdef"),
    }
    for what, (text, message) in cases.items():
        try:
            oracle_dump(text)
        except RuntimeError as e:
            assert message in str(e), (what, str(e))
        else:
            pytest.fail(f"{what}: the dump loaded")
    with pytest.raises(RuntimeError, match="truncated"):
        oracle_render(smoke[:1000], 8, 8, 1)
    with pytest.raises(RuntimeError, match="truncated"):
        oracle_trace_rays(smoke[:1000], np.zeros((1, 7)))


def test_a_dump_renders_in_pcg_mode_only():
    smoke = oracle_dump("7")
    for call in (lambda: oracle_render(smoke, 8, 8, 1, mode="mt"), lambda: oracle_render_adaptive(smoke, 12, 12, 1, mode="mt"),
                 lambda: oracle_render_images(smoke, 8, 8, 4, mode="mt"), lambda: oracle_probe(smoke, 2)):
        with pytest.raises(RuntimeError, match="pcg mode only"):
            call()
    assert oracle_render(smoke, 8, 8, 1, mode="pcg")["segments"] >= 64


def test_register_image_refuses_bad_arguments():
    assert oracle().orc_register_image(0, 4, 3, np.zeros(12, np.uint8).ctypes.data) != 0
    assert oracle().orc_register_image(2, 2, 5, np.zeros(20, np.uint8).ctypes.data) != 0
    assert oracle().orc_register_image(2, 2, 3, None) != 0


def test_loader_check_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/dump_loader_check.cpp linked with oracle/restate.cpp: good dumps, every truncation, the malformed cases."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("needs g++")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ lacks the AddressSanitizer / UBSan runtimes here")
    exe = tmp_path / "dump_loader_check"
    subprocess.run([cxx, "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-pthread", *flags, "-I", os.path.join(ROOT, "oracle"),
                    os.path.join(ROOT, "tests", "native", "dump_loader_check.cpp"), os.path.join(ROOT, "oracle", "restate.cpp"), "-lz",
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), ASSETS], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "dump loader ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------ recipes are not trivial
@pytest.mark.parametrize("name", list(recipes.RECIPES))
def test_recipe_is_not_trivial(options, name):
    recipe = recipes.RECIPES[name]
    W, H, spp = recipes.FRAME
    assert (W, H, spp) == (32, 18, 4)
    world, dump, kinds = recipes.compiled(recipe, options)
    frame = oracle_render(dump, W, H, spp)
    rays = recipes.pixel_centre_rays(recipe.view, W, H)
    assert len(rays) == 576
    t, _ = oracle_trace_rays(dump, rays)
    hit = np.isfinite(t)
    print(f"{name}: {hit.mean():.2f} of the camera rays hit, {frame['segments'] / (W * H * spp):.2f} segments per primary")
    assert hit.mean() >= 0.30
    assert frame["segments"] / (W * H * spp) >= 1.5
    assert {"lambertian"} < kinds and kinds & {"sphere", "triangle"}
    assert ("constant_medium" in kinds) == recipe.media
    for kind in sorted(kinds):
        # the world of this kind's primitives alone (the same coordinates): where it gives the full world's t, the kind is
        # what the ray hits first.  All media together: ray i's medium draws are then the full world's.
        _, only, _ = recipes.compiled(recipe, options, keep="constant_medium" if kind == "isotropic" else kind)
        t_kind, _ = oracle_trace_rays(only, rays)
        assert (hit & (bits(t_kind) == bits(t))).any(), kind


# ------------------------------------------------------------------------------------------------ coverage closure
# k_paths_g kernels that no GPU parity case runs: kernel -> the branch of launch_paths_g_ft no scene of reasonable size
# reaches.  LM 0 kernels only.  Empty: the `_wide` recipes reach LM 0 of every feature set (loose world-level spheres fill
# the LDS head until fewer than kLdsPartialMinNodes nodes fit: the last `go` of launch_paths_g_ft).
NOT_COMPARED = {}
# what tests/test_gpu_parity.py test_32bit_code_kernels_match_oracle_pcg pins with render.codes16 = 0: cow, dino, 8, 5
CODES16_OFF_KERNELS = {(39, 3, 2), (39, 3, 1), (125, 15, 1)}


def test_every_k_paths_g_kernel_in_the_library_has_a_parity_case():
    from tests.test_kernel_resources import LIB, SCENE_KERNELS, _paths_g, kernel_resources
    if not os.path.exists(LIB):
        pytest.skip("libart.so not built")
    built = set(_paths_g(kernel_resources.kernels(LIB)))
    recipe_kernels = {r.kernel for r in recipes.RECIPES.values()}
    claimed = set(SCENE_KERNELS.values()) | CODES16_OFF_KERNELS | recipe_kernels
    assert len(built) >= 45
    assert all(lm == 0 and reason for (_, _, lm), reason in NOT_COMPARED.items()), "NOT_COMPARED holds LM 0 kernels, each with its reason"
    assert not set(NOT_COMPARED) & claimed
    missing = built - claimed - set(NOT_COMPARED)
    assert not missing, f"k_paths_g kernels without an oracle parity case: {sorted(missing)}"
    assert all(k in recipe_kernels | set(SCENE_KERNELS.values()) for k in built if k[2] in (1, 2)), "every LM 1 / LM 2 kernel has a parity case that names it"
    assert recipe_kernels <= built, sorted(recipe_kernels - built)
