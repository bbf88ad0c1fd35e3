"""k_paths' first-bounce rounds (csrc/k_paths.hip, RayRing): a wave starts 64 paths at a time, traces and shades their
first segment together, writes the radiance of the paths that end there and appends the others, compacted, to its ring.

Every render here runs k_paths (extend_variant 3) and is bit-exact in the f64 sums, the RGB8 frame and the segment
count: builtin cameras against the oracle, custom cameras and worlds against the per-depth LDS kernel (wavefront,
variant 2) and the persistent kernel over the HBM scene (global_scene, variant 4), which this path start does not touch.
The cases are the batch outcomes: no entry appended (sky), every lane appended, max_depth 1 (the ring is never written)
and 2 (every entry is a last bounce), a light hit on the first segment, the pass ending inside a batch over several
passes, and the adaptive levels' entry-major slots.
"""
import numpy as np
import pytest

import another_raytracer_amd as art
from tests.oracle_lib import oracle_render, oracle_render_adaptive

pytestmark = pytest.mark.gpu


def render(objects, background, cam, W, H, spp, max_depth=50, seed=0, samples_per_pass=0, wavefront=False, global_scene=False):
    lookfrom, lookat, vup, vfov, aperture = cam
    c = art.camera(lookfrom, lookat, vup, vfov, W / H, aperture, 10.0, 0.0, 1.0)
    eng = art.engine(c, art.engine_mode.single, width=W, height=H, samples_per_pixel=spp, precision="f64", seed=seed,
                     max_depth=max_depth, samples_per_pass=samples_per_pass)
    eng.set_scene(objects, background)
    eng.wavefront = wavefront
    eng.global_scene = global_scene
    img = np.zeros((H, W, 3), np.uint8)
    acc = np.zeros((H, W, 3), np.float64)
    eng.run(img, accum=acc)
    return {"rgb": img, "acc": acc, "segments": eng.stats["segments"], "stats": eng.stats}


def builtin(scene, W, H, spp, **kw):
    world = art.scene_manager().build(scene)
    cam = (world.lookfrom, world.lookat, (0, 1, 0), world.vfov, world.aperture)
    return render(world.objects, world.background, cam, W, H, spp, **kw)


def same(a, b):
    return a["acc"].tobytes() == b["acc"].tobytes() and np.array_equal(a["rgb"], b["rgb"]) and a["segments"] == b["segments"]


def check_against_other_kernels(objects, background, cam, W, H, spp, **kw):
    """k_paths against the per-depth LDS kernel and the HBM persistent kernel on the same scene and camera."""
    a = render(objects, background, cam, W, H, spp, **kw)
    b = render(objects, background, cam, W, H, spp, wavefront=True, **kw)
    c = render(objects, background, cam, W, H, spp, global_scene=True, **kw)
    assert a["stats"]["extend_variant"] == 3, a["stats"]
    assert b["stats"]["extend_variant"] == 2, b["stats"]
    assert c["stats"]["extend_variant"] == 4, c["stats"]
    print(f"segments {a['segments']} / {b['segments']} / {c['segments']} for {W * H * spp} paths")
    assert same(a, b)
    assert same(a, c)
    return a


def test_sky_batches_append_nothing(gpu):
    # the benchmark scene seen from above its spheres, looking up: every camera ray misses, so no batch appends an
    # entry and the loop only drains; 72x40: partial 8x8 tiles
    W, H, spp = 72, 40, 5
    world = art.scene_manager().build("1")
    cam = ((13.0, 3.0, 3.0), (13.0, 100.0, 30.0), (0, 1, 0), 20.0, world.aperture)
    a = check_against_other_kernels(world.objects, world.background, cam, W, H, spp)
    assert a["segments"] == W * H * spp  # the case is the one meant: every path is one segment
    assert a["rgb"].min() > 0  # sky, not an empty frame


def test_full_batches(gpu):
    # from above the ground, looking down with a narrow field of view: every camera ray hits, whole 8x8 tiles, so the
    # batches append (nearly) all 64 lanes and the ring runs full
    W, H, spp = 64, 40, 6
    world = art.scene_manager().build("1")
    cam = ((0.3, 30.0, 0.2), (0.5, 0.0, 0.3), (0, 0, -1), 10.0, world.aperture)
    a = check_against_other_kernels(world.objects, world.background, cam, W, H, spp, max_depth=50)
    assert a["segments"] >= 2 * W * H * spp  # the paths go on after the first bounce


@pytest.mark.parametrize("max_depth", [1, 2])
@pytest.mark.parametrize("W,H,spp", [(13, 70, 2), (130, 2, 5)])
def test_short_paths(gpu, W, H, spp, max_depth):
    # max_depth 1: every path ends in its batch, the ring is never written; 2: every ring entry is a last bounce
    g = builtin("1", W, H, spp, max_depth=max_depth)
    o = oracle_render("1", W, H, spp, mode="pcg", max_depth=max_depth)
    assert g["stats"]["extend_variant"] == 3
    assert np.array_equal(g["acc"], o["acc"]) and np.array_equal(g["rgb"], o["rgb"])
    assert g["segments"] == o["segments"]
    if max_depth == 1:
        assert g["segments"] == W * H * spp


def light_world():
    art.reset_scene_rng()
    objects = art.hittable_list()
    objects.add(art.sphere((0, -1000, 0), 1000, art.lambertian(art.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))))
    objects.add(art.sphere((-2.2, 1.0, 0.0), 1.0, art.lambertian((0.4, 0.2, 0.1))))
    objects.add(art.sphere((0.0, 1.0, 0.0), 1.0, art.dielectric(1.5)))
    objects.add(art.sphere((2.2, 1.0, 0.0), 1.0, art.metal((0.7, 0.6, 0.5), 0.0)))
    # fuzz 1 on a sphere seen at grazing angles and from behind the others: some reflected rays point inwards and are absorbed
    objects.add(art.sphere((0.0, 0.6, -3.0), 0.6, art.metal((0.8, 0.8, 0.9), 1.0)))
    objects.add(art.moving_sphere((-1.0, 0.3, 2.0), (-1.0, 0.7, 2.0), 0.0, 1.0, 0.3, art.lambertian((0.1, 0.3, 0.8))))
    objects.add(art.sphere((1.0, 2.6, 1.5), 0.5, art.diffuse_light((7.0, 6.0, 5.0))))  # in direct view
    world = art.hittable_list()
    world.add(art.bvh_node(objects, 0, 1))
    return world


@pytest.mark.parametrize("max_depth", [50, 1])
def test_light_hit_on_the_first_segment(gpu, max_depth):
    # black background: every non-zero sum comes from the light; its direct view ends paths in the batch with radiance
    W, H, spp = 40, 24, 6
    cam = ((0.0, 3.0, 9.0), (0.0, 1.2, 0.0), (0, 1, 0), 40.0, 0.05)
    a = check_against_other_kernels(light_world(), (0.0, 0.0, 0.0), cam, W, H, spp, max_depth=max_depth)
    art.reset_scene_rng()
    direct = (a["acc"] == np.array([7.0, 6.0, 5.0]) * spp).all(axis=-1)
    assert direct.any()  # pixels whose every sample saw the light first
    if max_depth == 1:
        assert a["segments"] == W * H * spp
        lit = a["acc"].reshape(-1, 3)
        assert ((lit == 0).all(axis=1) | (lit[:, 0] > 0)).all() and (lit == 0).all(axis=1).any()
    else:
        assert a["segments"] > W * H * spp and ((a["acc"] > 0).any(axis=-1) & ~direct).any()  # and lit through bounces


def test_pass_end_inside_a_batch_over_several_passes(gpu):
    # 100x52: 13 x 7 tiles of which the last column and row are partial; 5 + 5 + 2 samples against one pass of 12
    W, H, spp = 100, 52, 12
    many = builtin("1", W, H, spp, seed=1, samples_per_pass=5)
    one = builtin("1", W, H, spp, seed=1)
    o = oracle_render("1", W, H, spp, mode="pcg", seed=1)
    assert many["stats"]["passes"] == 3 and one["stats"]["passes"] == 1
    assert many["stats"]["extend_variant"] == 3 and one["stats"]["extend_variant"] == 3
    assert same(many, one)
    assert np.array_equal(one["acc"], o["acc"]) and np.array_equal(one["rgb"], o["rgb"]) and one["segments"] == o["segments"]


def test_entry_major_slots(gpu):
    # the adaptive levels' passes: a batch is 64 consecutive samples of the list's entries (slot = entry * k + sample)
    W, H, spp = 36, 24, 3
    world = art.scene_manager().build("1")
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    eng = art.engine(cam, art.engine_mode.adaptive, width=W, height=H, samples_per_pixel=spp, seed=0)
    eng.set_scene(world.objects, world.background)
    img = np.zeros((H, W, 3), np.uint8)
    eng.run(img)
    o = oracle_render_adaptive("1", W, H, spp, mode="pcg")
    assert eng.stats["extend_variant"] == 3
    assert np.array_equal(img, o["rgb"])
    assert eng.stats["segments"] == o["segments"]
