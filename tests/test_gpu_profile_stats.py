"""RT_PROFILE's launch accounting (rt_stats.extend_ms / shade_ms / extend_launches / shade_launches) for every way the
renderer runs a pass: the persistent kernels (k_paths, k_paths_g), the per-depth wavefront variants, both adaptive forms
and the noise-target rounds.  Profiling only records events around the launches: the image with it equals the image
without it bit for bit, and the launch counts follow from the pass count, the depth and the variant.  A persistent launch has
no shade interval: shade_ms is exactly 0 there (a build that brackets an empty interval with two event records reports the
5-10 us between them instead)."""
import functools

import numpy as np
import pytest

import another_raytracer_amd as art

pytestmark = pytest.mark.gpu

SPP, DEPTH, SEED = 4, 6, 3
FRAME = {"1": (48, 36), "cow": (32, 18)}  # 48x36: adaptive's 12-pixel squares fit


@functools.lru_cache(maxsize=None)
def world_of(scene):
    return art.scene_manager().build(scene)


def engine(scene, mode=art.engine_mode.single, spp=SPP, samples_per_pass=0, **switches):
    W, H = FRAME[scene]
    world = world_of(scene)
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    eng = art.engine(cam, mode, width=W, height=H, samples_per_pixel=spp, max_depth=DEPTH, seed=SEED, samples_per_pass=samples_per_pass)
    eng.set_scene(world.objects, world.background)
    for name, value in switches.items():
        setattr(eng, name, value)
    return eng


def render(scene, profile, **kw):
    eng = engine(scene, **kw)
    W, H = FRAME[scene]
    img = np.zeros((H, W, 3), np.uint8)
    eng.run(img, profile=profile)
    return img, dict(eng.stats)


def profiled(scene, **kw):
    """The stats of the profiled render, after the checks every case shares."""
    img0, st0 = render(scene, False, **kw)
    img1, st1 = render(scene, True, **kw)
    assert np.array_equal(img0, img1)
    assert st0["extend_ms"] == 0 and st0["shade_ms"] == 0 and st0["extend_launches"] == 0 and st0["shade_launches"] == 0
    assert st1["extend_ms"] > 0
    for key in ("passes", "samples_per_pass", "segments", "primary", "extend_variant"):
        assert st0[key] == st1[key], key
    return img1, st1


@pytest.mark.parametrize("scene,variant", [("1", 3), ("cow", 4)])
@pytest.mark.parametrize("samples_per_pass,passes", [(0, 1), (2, 2)])
def test_persistent_render(scene, variant, samples_per_pass, passes):
    _, st = profiled(scene, samples_per_pass=samples_per_pass)
    assert st["extend_variant"] == variant and st["passes"] == passes
    assert st["extend_launches"] == passes
    assert st["shade_launches"] == 0 and st["shade_ms"] == 0


@pytest.mark.parametrize("samples_per_pass,passes", [(0, 1), (2, 2)])
def test_fused_wavefront(samples_per_pass, passes):
    _, st = profiled("1", samples_per_pass=samples_per_pass, wavefront=True)
    assert st["extend_variant"] == 2 and st["passes"] == passes
    assert st["extend_launches"] == passes * DEPTH
    assert st["shade_launches"] == 0


@pytest.mark.parametrize("scene,switch,variant", [("1", "split_shade", 1), ("cow", "wavefront", 0)])
@pytest.mark.parametrize("samples_per_pass,passes", [(0, 1), (2, 2)])
def test_split_shade_wavefront(scene, switch, variant, samples_per_pass, passes):
    _, st = profiled(scene, samples_per_pass=samples_per_pass, **{switch: True})
    assert st["extend_variant"] == variant and st["passes"] == passes
    assert st["extend_launches"] == passes * DEPTH and st["shade_launches"] == passes * DEPTH
    assert st["shade_ms"] > 0


def test_adaptive_both_level_counts():
    dev_img, dev = profiled("1", mode=art.engine_mode.adaptive)  # one pass per level, counted on the device
    assert dev["passes"] == 4 and dev["extend_launches"] == 4 and dev["shade_launches"] == 0
    host_img, host = profiled("1", mode=art.engine_mode.adaptive, samples_per_pass=2)  # counted on the host
    assert host["passes"] >= 4 and host["extend_launches"] == host["passes"] and host["shade_launches"] == 0
    assert np.array_equal(host_img, dev_img)
    assert host["primary"] == dev["primary"] and host["segments"] == dev["segments"]


def test_noise_target_rounds():
    """Base passes of k samples, then every round's sub-passes: a round of n_active pixels and k_next samples runs in
    ceil(k_next / min(k_next, Pmax / n_active)) launches, Pmax = k * padded pixels."""
    W, H = FRAME["1"]
    cap, min_spp, step = 12, 4, 4
    out = {}
    for profile in (False, True):
        eng = engine("1", spp=cap, samples_per_pass=2)
        img = np.zeros((H, W, 3), np.uint8)
        count = np.zeros((H, W), np.int32)
        res = eng.run_noise_target(img, counts=count, min_spp=min_spp, step_spp=step, rel_tol=0.02, profile=profile)
        out[profile] = (img, count, res, dict(eng.stats))
    (img0, count0, res0, st0), (img1, count1, res1, st) = out[False], out[True]
    assert np.array_equal(img0, img1) and np.array_equal(count0, count1)
    assert res0["rounds"] == res1["rounds"] and res0["samples"] == res1["samples"]
    assert st0["extend_ms"] == 0 and st0["extend_launches"] == 0 and st0["passes"] == st["passes"]
    k = st["samples_per_pass"]
    assert k == 2
    pmax = k * ((W + 7) // 8) * ((H + 7) // 8) * 64
    expected = -(-min_spp // k)
    done = min_spp
    while done < cap:
        n_active = int((count1 > done).sum())
        if n_active == 0:
            break
        k_next = min(step, cap - done)
        expected += -(-k_next // min(k_next, pmax // n_active))
        done += k_next
    assert res1["rounds"] >= 1 and expected > -(-min_spp // k)
    assert st["passes"] == expected and st["extend_launches"] == expected
    assert st["extend_ms"] > 0 and st["shade_launches"] == 0 and st["shade_ms"] == 0
