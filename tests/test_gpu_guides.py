"""First-hit guide buffers (rt_render_guides, k_guides): t and normal equal rt_trace_rays of the pixel-centre rays bit for
bit on every builtin scene, position is the hit point, albedo the first hit's material colour; band sets and the HBM
traversal give the whole frame's records."""
import ctypes
import functools

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import check, lib

pytestmark = pytest.mark.gpu

SCENES = ["1", "2", "3", "4", "5", "6", "7", "8", "9", "c1", "cow", "dino"]


def make_engine(world, W, H, objects=None, background=None):
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=2)
    eng.set_scene(world.objects if objects is None else objects, world.background if background is None else background)
    return eng


@functools.lru_cache(maxsize=None)
def frame(scene, W, H):
    """(world, engine, guides, rays) of a builtin scene's whole frame, computed once."""
    world = art.scene_manager().build(scene)
    eng = make_engine(world, W, H)
    rays = np.zeros((H, W, 7))
    guides = eng.render_guides(rays=rays)
    guides.setflags(write=False)
    rays.setflags(write=False)
    return world, eng, guides, rays


def same_bits(a, b):
    # any NaN equals any NaN (tests/test_gpu_rays.py: a ray in a rect's plane has t = 0/0)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("scene,W,H", [(s, 64, 36) for s in SCENES] + [("8", 37, 23)])
def test_guides_equal_the_ray_query_of_their_own_rays(gpu, scene, W, H):
    world, eng, guides, rays = frame(scene, W, H)
    n = W * H
    t = np.zeros(n)
    nrm = np.zeros((n, 3))
    flat = np.ascontiguousarray(rays.reshape(n, 7))
    check(lib.rt_trace_rays(eng._scene, flat.ctypes.data_as(ctypes.c_void_p), n, 0, t.ctypes.data_as(ctypes.c_void_p),
                            nrm.ctypes.data_as(ctypes.c_void_p)), "rt_trace_rays")
    g = guides.reshape(n, 10)
    assert same_bits(np.ascontiguousarray(g[:, 9]), t).all()
    assert same_bits(np.ascontiguousarray(g[:, 3:6]), nrm).all()
    # the rays: from lookfrom exactly (no lens offset), at time0
    assert (flat[:, 0:3] == np.array(world.lookfrom, float)).all()
    assert (flat[:, 6] == 0.0).all()
    hit = np.isfinite(t)
    assert hit.any()
    # position is the hit point: o + t d up to the rounding of a transform round trip
    p = g[hit, 6:9]
    want = flat[hit, 0:3] + t[hit, None] * flat[hit, 3:6]
    assert (np.abs(p - want) <= 1e-9 * (1.0 + np.abs(p))).all()
    # a miss: t = +inf, normal 0, position +inf, albedo 1
    miss = np.isposinf(t)
    assert (g[miss, 3:6] == 0.0).all() and np.isposinf(g[miss, 6:9]).all() and (g[miss, 0:3] == 1.0).all()
    assert np.isfinite(g[:, 0:3]).all() and (g[:, 0:3] >= 0.0).all()


def test_rays_go_through_the_pixel_centres(gpu):
    # the ray of pixel (i, j) is the camera's ray at s = (i + 0.5) / (W - 1), t = ((H - 1 - j) + 0.5) / (H - 1): the
    # directions are affine in (i, j), and neighbouring pixels differ by horizontal / (W - 1) and vertical / (H - 1)
    W, H = 64, 36
    _, _, _, rays = frame("1", W, H)
    d = rays[..., 3:6]
    dx = d[:, 1:] - d[:, :-1]
    dy = d[1:] - d[:-1]
    assert np.allclose(dx, dx[0, 0], rtol=0, atol=1e-12) and np.allclose(dy, dy[0, 0], rtol=0, atol=1e-12)
    # the frame's centre (between the four middle pixels, half a pixel off the lattice) looks at lookat
    world = frame("1", W, H)[0]
    look = np.array(world.lookat, float) - np.array(world.lookfrom, float)
    i_mid, j_mid = 0.5 * (W - 1) - 0.5, 0.5 * (H - 1) + 0.5  # pixel coordinates where s = t = 0.5
    mid = d[0, 0] + i_mid * dx[0, 0] + j_mid * dy[0, 0]
    cosine = mid @ look / (np.linalg.norm(mid) * np.linalg.norm(look))
    assert cosine > 1.0 - 1e-9


def test_band_sets_equal_the_whole_frames_rows(gpu):
    W, H = 64, 36
    _, eng, guides, rays = frame("8", W, H)
    seen = np.zeros(H, bool)
    for r in range(3):
        rows = eng.local_rows(8, 3, r)
        band_rays = np.zeros((len(rows), W, 7))
        band = eng.render_guides(rays=band_rays, band_rows=8, band_count=3, band_index=r)
        assert band.shape == (len(rows), W, 10)
        assert same_bits(np.ascontiguousarray(band), np.ascontiguousarray(guides[rows])).all()
        assert same_bits(band_rays, np.ascontiguousarray(rays[rows])).all()
        seen[rows] = True
    assert seen.all()


def test_global_scene_equals_the_lds_image(gpu):
    W, H = 64, 36
    world, eng, guides, _ = frame("1", W, H)
    hbm = make_engine(world, W, H)
    hbm.global_scene = True
    assert same_bits(hbm.render_guides(), np.ascontiguousarray(guides)).all()


def test_device_buffers_receive_the_same_records(gpu):
    import torch
    W, H = 37, 23
    _, eng, guides, rays = frame("8", W, H)
    g = torch.zeros((H, W, 10), dtype=torch.float64, device="cuda")
    r = torch.zeros((H, W, 7), dtype=torch.float64, device="cuda")
    eng.render_guides(guides=g, rays=r)
    assert same_bits(g.cpu().numpy(), np.ascontiguousarray(guides)).all()
    assert same_bits(r.cpu().numpy(), np.ascontiguousarray(rays)).all()


@pytest.mark.parametrize("scene", ["1", "cow"])
def test_device_buffers_on_a_side_stream_receive_the_same_records(gpu, scene):
    # device buffers written in place on the caller's stream (the call waits all the same); the host frame is the reference
    import torch
    W, H = 37, 23
    _, eng, guides, rays = frame(scene, W, H)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.zeros((H, W, 10), dtype=torch.float64, device="cuda")
        r = torch.zeros((H, W, 7), dtype=torch.float64, device="cuda")
        eng.render_guides(guides=g, rays=r, stream=side.cuda_stream)
        got_g, got_r = g.cpu().numpy(), r.cpu().numpy()
    assert same_bits(got_g, np.ascontiguousarray(guides)).all()
    assert same_bits(got_r, np.ascontiguousarray(rays)).all()


def test_albedo_is_the_first_hits_material_colour(gpu):
    art.reset_scene_rng()
    red, green, blue, steel = (0.8, 0.1, 0.15), (0.2, 0.7, 0.25), (0.1, 0.3, 0.9), (0.6, 0.55, 0.4)
    spheres = [((-3.0, 1.0, 0.0), 1.0, red), ((-1.0, 1.0, 0.0), 0.8, green), ((0.0, -1000.0, 0.0), 1000.0, blue), ((1.0, 1.0, 0.0), 0.8, steel),
               ((3.0, 1.0, 0.0), 1.0, (1.0, 1.0, 1.0))]
    world = art.hittable_list()
    world.add(art.sphere(*spheres[0][:2], art.lambertian(red)))
    world.add(art.sphere(*spheres[1][:2], art.lambertian(green)))
    world.add(art.sphere(*spheres[2][:2], art.lambertian(blue)))
    world.add(art.sphere(*spheres[3][:2], art.metal(steel, 0.1)))
    world.add(art.sphere(*spheres[4][:2], art.dielectric(1.5)))
    light_y = 4.0
    world.add(art.xz_rect(-2.0, 2.0, -1.0, 1.0, light_y, art.diffuse_light((7.0, 6.0, 5.0))))
    W, H = 64, 36
    cam = art.camera((0.0, 3.0, 9.0), (0.0, 1.5, 0.0), (0, 1, 0), 50.0, W / H, 0.0, 10.0, 0.0, 1.0)
    eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=2)
    eng.set_scene(world, (0.5, 0.7, 1.0))
    g = eng.render_guides().reshape(-1, 10)
    hit = np.isfinite(g[:, 9])
    pos, alb = g[:, 6:9], g[:, 0:3]
    owner = np.full(len(g), -1)
    for k, (c, r, _) in enumerate(spheres):
        on = hit & (np.abs(np.linalg.norm(pos - np.array(c), axis=1) - r) <= 1e-9 * (1.0 + r))
        assert (owner[on] == -1).all()
        owner[on] = k
    on = hit & (pos[:, 1] == light_y)
    assert (owner[on] == -1).all()
    owner[on] = len(spheres)
    assert (owner[hit] >= 0).all()
    colours = [s[2] for s in spheres] + [(1.0, 1.0, 1.0)]
    for k, colour in enumerate(colours):
        assert (owner == k).sum() > 0, k  # every object is in the frame
        assert (alb[owner == k] == np.array(colour)).all(), k
    assert (~hit).any() and (alb[~hit] == 1.0).all()


def test_checker_albedo_is_one_of_its_two_colours(gpu):
    _, _, guides, _ = frame("2", 64, 36)
    g = guides.reshape(-1, 10)
    hit = np.isfinite(g[:, 9])
    even, odd = np.array([0.2, 0.3, 0.1]), np.array([0.9, 0.9, 0.9])
    is_even = (g[hit, 0:3] == even).all(axis=1)
    is_odd = (g[hit, 0:3] == odd).all(axis=1)
    assert (is_even | is_odd).all() and is_even.any() and is_odd.any()
