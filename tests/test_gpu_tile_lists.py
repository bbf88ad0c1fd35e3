"""k_paths' per-tile sphere lists (csrc/tile_lists.h, tile_lists.hip, k_paths.hip trace_tile_list; option
render.tile_lists): a batch of 64 camera rays tests the few spheres its 8x8 tile can reach instead of walking the tree.

Every render here runs k_paths (extend_variant 3) with the lists forced on (option 2) and is compared with the same render
without them (option 0), and with the oracle where a builtin scene and camera allow: the RGB8 frame, the f64 sums and the
segment count are bit-identical.  engine.tile_candidates (rt_tile_candidates) shows which path the tiles took.  Scene 1
holds moving spheres (every lambertian sphere has a moving twin), so its cases are the moving-sphere cases too.
"""
import functools

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd.distributed import band_rows_of
from tests.oracle_lib import oracle_render, oracle_render_adaptive

pytestmark = pytest.mark.gpu
OVERFLOW = 0xFFFF


def render(objects, background, cam, W, H, spp, lists, max_depth=50, samples_per_pass=0, wavefront=False, global_scene=False,
           bands=None, mode=None):
    """One render under option render.tile_lists = lists; bands = (band_rows, band_count, band_index)."""
    lookfrom, lookat, vup, vfov, aperture = cam
    c = art.camera(lookfrom, lookat, vup, vfov, W / H, aperture, 10.0, 0.0, 1.0)
    eng = art.engine(c, mode or art.engine_mode.single, width=W, height=H, samples_per_pixel=spp, precision="f64", seed=0,
                     max_depth=max_depth, samples_per_pass=samples_per_pass)
    eng.set_scene(objects, background)
    eng.wavefront = wavefront
    eng.global_scene = global_scene
    kw = dict(band_rows=bands[0], band_count=bands[1], band_index=bands[2]) if bands else {}
    rows = len(band_rows_of(H, *bands)) if bands else H
    img = np.zeros((rows, W, 3), np.uint8)
    acc = None if mode == art.engine_mode.adaptive else np.zeros((rows, W, 3), np.float64)
    art.set_option("render.tile_lists", lists)
    try:
        tiles = eng.tile_candidates(**kw)
        eng.run(img, accum=acc, **kw)
    finally:
        art.set_option(None, 0)
    return {"rgb": img, "acc": acc, "segments": eng.stats["segments"], "stats": eng.stats, "tiles": tiles}


@functools.lru_cache(maxsize=None)
def scene1(W, H, spp, lists, aperture=None, **kw):
    world = art.scene_manager().build("1")
    cam = (world.lookfrom, world.lookat, (0, 1, 0), world.vfov, world.aperture if aperture is None else aperture)
    g = render(world.objects, world.background, cam, W, H, spp, lists, **kw)
    assert g["stats"]["extend_variant"] == 3, g["stats"]
    return g


@functools.lru_cache(maxsize=None)
def oracle(W, H, spp, max_depth=50):
    return oracle_render("1", W, H, spp, mode="pcg", max_depth=max_depth)


def same(a, b):
    return a["acc"].tobytes() == b["acc"].tobytes() and np.array_equal(a["rgb"], b["rgb"]) and a["segments"] == b["segments"]


def kinds(tiles):
    return int((tiles != OVERFLOW).sum()), int((tiles == OVERFLOW).sum())


def test_scene1_listed_and_overflow_tiles(gpu):
    W, H, spp = 256, 144, 2
    on, off = scene1(W, H, spp, 2), scene1(W, H, spp, 0)
    assert off["tiles"] is None and on["tiles"].shape == (18, 32)
    listed, over = kinds(on["tiles"])
    print(f"{W}x{H}: {listed} listed tiles (mean {on['tiles'][on['tiles'] != OVERFLOW].mean():.2f} spheres), {over} overflow tiles")
    assert listed > 0 and over > 0  # both paths ran
    assert same(on, off)
    assert same(on, oracle(W, H, spp))


@pytest.mark.parametrize("W,H,spp", [(72, 40, 3), (5, 3, 2)])
def test_partial_tiles_and_less_than_one_batch(gpu, W, H, spp):
    on = scene1(W, H, spp, 2)
    assert on["tiles"] is not None and on["tiles"].shape == ((H + 7) // 8, (W + 7) // 8)
    assert same(on, scene1(W, H, spp, 0))
    assert same(on, oracle(W, H, spp))


def mirror_room():
    """tests/test_gpu_path_pool.py's closed room: the camera sits inside a fuzz-0 metal sphere that nothing leaves, so a
    path ends only on the light or at max_depth; five spheres, so every tile is listed, and the room's wall is a
    candidate of every tile."""
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


def test_mirror_room_camera_inside_a_sphere(gpu):
    W, H, spp = 64, 40, 6
    cam = ((0.0, 1.0, 8.0), (0.0, 1.5, 0.0), (0, 1, 0), 70.0, 0.0)
    world = mirror_room()
    bg = (0.0, 0.0, 0.0)
    a = render(world, bg, cam, W, H, spp, 2)
    z = render(world, bg, cam, W, H, spp, 0)
    b = render(world, bg, cam, W, H, spp, 2, wavefront=True)
    c = render(world, bg, cam, W, H, spp, 2, global_scene=True)
    art.reset_scene_rng()
    assert a["stats"]["extend_variant"] == 3 and b["stats"]["extend_variant"] == 2 and c["stats"]["extend_variant"] == 4
    assert b["tiles"] is None and c["tiles"] is None  # only k_paths reads lists
    t = a["tiles"]
    assert t is not None and (t >= 1).all() and (t <= 5).all(), t  # every tile listed, the wall in every list
    assert a["segments"] > 5 * W * H * spp  # deep paths (the path-pool test's argument)
    assert same(a, z) and same(a, b) and same(a, c)


@pytest.mark.parametrize("aperture,W,H", [(0.0, 72, 40), (1.0, 256, 144)])
def test_aperture_zero_and_large(gpu, aperture, W, H):
    # aperture 1: a lens ten times the scene's, of radius 0.5.  At 72x40 its bundles are so wide that every tile
    # overflows (measured with aperture 2: 45 of 45); at 256x144 the rays of the top rows, which leave the lens 1.5 above
    # the ground and rise, clear every sphere (tops at 0.9), so those tiles are listed: both paths run
    spp = 2
    on, off = scene1(W, H, spp, 2, aperture=aperture), scene1(W, H, spp, 0, aperture=aperture)
    listed, over = kinds(on["tiles"])
    print(f"aperture {aperture}: {listed} listed, {over} overflow")
    assert listed > 0
    assert same(on, off)


def test_bands_against_the_unbanded_frame(gpu):
    W, H, spp = 72, 40, 2
    whole = scene1(W, H, spp, 0)
    rgb, acc, segs = np.zeros_like(whole["rgb"]), np.zeros_like(whole["acc"]), 0
    for bi in range(3):
        g = scene1(W, H, spp, 2, bands=(4, 3, bi))
        rows = band_rows_of(H, 4, 3, bi)
        assert g["tiles"] is not None and g["tiles"].shape == ((len(rows) + 7) // 8, 9)
        rgb[rows], acc[rows] = g["rgb"], g["acc"]
        segs += g["segments"]
    assert same({"rgb": rgb, "acc": acc, "segments": segs}, whole)


def test_several_passes_equal_one(gpu):
    W, H, spp = 72, 40, 3
    many = scene1(W, H, spp, 2, samples_per_pass=1)
    assert many["stats"]["passes"] == 3
    assert same(many, scene1(W, H, spp, 2))


@pytest.mark.parametrize("max_depth", [1, 2])
def test_short_paths(gpu, max_depth):
    W, H, spp = 72, 40, 3
    on = scene1(W, H, spp, 2, max_depth=max_depth)
    assert same(on, scene1(W, H, spp, 0, max_depth=max_depth))
    assert same(on, oracle(W, H, spp, max_depth))


def test_adaptive_list_mode_ignores_the_table(gpu):
    W, H, spp = 36, 24, 3
    world = art.scene_manager().build("1")
    cam = (world.lookfrom, world.lookat, (0, 1, 0), world.vfov, world.aperture)
    g = render(world.objects, world.background, cam, W, H, spp, 2, mode=art.engine_mode.adaptive)
    o = oracle_render_adaptive("1", W, H, spp, mode="pcg")
    assert g["stats"]["extend_variant"] == 3 and g["tiles"] is None
    assert np.array_equal(g["rgb"], o["rgb"]) and g["segments"] == o["segments"]


def test_auto_mode_builds_no_table_at_a_small_sample_count(gpu):
    W, H, spp = 72, 40, 3
    auto = scene1(W, H, spp, 1)
    assert auto["tiles"] is None  # 3 samples per pass: below the threshold
    assert same(auto, scene1(W, H, spp, 0))
    # and at the threshold the table is built (the lists only, no render)
    world = art.scene_manager().build("1")
    c = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    eng = art.engine(c, art.engine_mode.single, width=W, height=H, samples_per_pixel=72)
    eng.set_scene(world.objects, world.background)
    assert art.get_option("render.tile_lists") == 1
    assert eng.tile_candidates() is not None
