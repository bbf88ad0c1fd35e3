"""k_paths' per-wave path pool (csrc/k_paths.hip, PathPool; csrc/path_pool.h): a batch of 64 camera rays overwrites
every lane, the paths the lanes held are pushed, compacted, onto a LIFO pool, the batch's survivors stay in their lanes
and idle lanes pop the pool in ordinary rounds.

Every render here runs k_paths (extend_variant 3) and is bit-exact in the f64 sums, the RGB8 frame and the segment
count: builtin cameras against the oracle, the custom world against the per-depth LDS kernel (wavefront, variant 2) and
the persistent kernel over the HBM scene (global_scene, variant 4), which have no pool.  The cases: entries that stay at
the pool's bottom across many batches (long paths among short ones), fewer slots than one batch, a pass that ends with
paths in the pool (one pass and several), max_depth 2 and 3 (every popped entry is a last or next-to-last bounce), and
the adaptive levels' entry-major slots.
"""
import functools

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
    g = render(world.objects, world.background, cam, W, H, spp, **kw)
    assert g["stats"]["extend_variant"] == 3, g["stats"]
    return g


@functools.lru_cache(maxsize=None)
def oracle(W, H, spp, max_depth=50):
    return oracle_render("1", W, H, spp, mode="pcg", max_depth=max_depth)


def same(a, b):
    return a["acc"].tobytes() == b["acc"].tobytes() and np.array_equal(a["rgb"], b["rgb"]) and a["segments"] == b["segments"]


def mirror_room():
    """A closed room: the camera sits inside a fuzz-0 metal sphere that nothing leaves, so a path ends only on the light
    or at max_depth.  The light fills a few percent of the directions seen from the room's wall and the spheres, so path
    lengths spread from 1 (the light in direct view) to max_depth: a wave holds old deep paths among new short ones."""
    art.reset_scene_rng()
    objects = art.hittable_list()
    objects.add(art.sphere((0.0, 0.0, 0.0), 12.0, art.metal((0.95, 0.95, 0.95), 0.0)))
    objects.add(art.sphere((0.0, -4.0, 0.0), 2.5, art.lambertian((0.7, 0.6, 0.5))))
    objects.add(art.sphere((-4.5, 1.0, -2.0), 1.5, art.dielectric(1.5)))
    objects.add(art.sphere((4.5, 1.0, -2.0), 1.5, art.metal((0.8, 0.8, 0.9), 0.0)))
    objects.add(art.sphere((0.0, 7.0, 0.0), 3.0, art.diffuse_light((4.0, 4.0, 4.0))))
    world = art.hittable_list()
    world.add(art.bvh_node(objects, 0, 1))
    return world


def test_deep_entries_under_many_batches(gpu):
    W, H, spp = 64, 40, 6
    cam = ((0.0, 1.0, 8.0), (0.0, 1.5, 0.0), (0, 1, 0), 70.0, 0.0)
    kw = dict(max_depth=50)
    world = mirror_room()
    a = render(world, (0.0, 0.0, 0.0), cam, W, H, spp, **kw)
    b = render(world, (0.0, 0.0, 0.0), cam, W, H, spp, wavefront=True, **kw)
    c = render(world, (0.0, 0.0, 0.0), cam, W, H, spp, global_scene=True, **kw)
    art.reset_scene_rng()
    assert a["stats"]["extend_variant"] == 3 and b["stats"]["extend_variant"] == 2 and c["stats"]["extend_variant"] == 4
    paths = W * H * spp
    print(f"segments per path: {a['segments'] / paths:.2f} / {b['segments'] / paths:.2f} / {c['segments'] / paths:.2f}")
    # The case is the one meant, by the reference renders' own count: no path leaves the room, and one bounce ends on
    # the light with a probability of a few percent (its share of the directions: (3 / 8)^2 / 4 = 0.035 from 8 units
    # away), at most 0.15 anywhere, so the mean length is at least (1 - 0.85^50) / 0.15 = 6.7 segments; a path whose
    # camera ray sees the light has one.  More than 5 segments per path means that deep paths lie under the short ones.
    assert b["segments"] == c["segments"] and b["segments"] > 5 * paths
    assert same(a, b)
    assert same(a, c)
    assert (a["acc"] > 0).any()


@pytest.mark.parametrize("W,H,spp", [(5, 3, 2), (8, 8, 1)])
def test_fewer_slots_than_one_batch(gpu, W, H, spp):
    # the first batch is partial (5x3: one padded 8x8 tile per sample) or exactly full, and the pass is exhausted at
    # once with its paths in flight
    g = builtin("1", W, H, spp)
    assert same(g, oracle(W, H, spp))


def test_pass_exhausted_with_paths_in_the_pool(gpu):
    # 64x32: 2048 slots per sample, a multiple of the batch and of the slot chunk, so a wave's last batch is full and
    # the paths it displaced are popped after the pass is exhausted; several passes equal one
    W, H = 64, 32
    assert same(builtin("1", W, H, 1), oracle(W, H, 1))
    one = builtin("1", W, H, 3)
    many = builtin("1", W, H, 3, samples_per_pass=1)
    assert one["stats"]["passes"] == 1 and many["stats"]["passes"] == 3
    assert same(many, one)
    assert same(one, oracle(W, H, 3))


@pytest.mark.parametrize("max_depth", [2, 3])
def test_short_paths_through_the_pool(gpu, max_depth):
    # every popped entry is a last (max_depth 2) or a last or next-to-last (3) bounce; 72x40: partial tiles
    W, H, spp = 72, 40, 3
    g = builtin("1", W, H, spp, max_depth=max_depth)
    o = oracle(W, H, spp, max_depth)
    assert same(g, o)
    assert W * H * spp < g["segments"] <= max_depth * W * H * spp


def test_adaptive_entry_major_slots(gpu):
    # the adaptive levels' passes: a batch is 64 consecutive samples of the list's entries (one pixel's samples)
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
