"""rt_render_views on the GPU: every view of one call equals rt_render (engine.run) with that view's camera and seed, bit
for bit -- the RGB8 frame, the f64 sums and, summed over the views, the segment count.  Checked on the LDS-image and the
HBM forms of the path kernel, with one seed for all views, at a size where every lane of the persistent grid refills,
with the views cut into several launches, at one sample and at depth one, and on host against device buffers."""
import functools
import math

import numpy as np
import pytest

import another_raytracer_amd as art

pytestmark = pytest.mark.gpu

W, H, SPP = 40, 24, 4  # neither side a multiple of 8; 3840 paths a view, no multiple of a wave's 64 lanes per row
SEED0 = 3


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@functools.lru_cache(maxsize=None)
def world_of(scene):
    return art.scene_manager().build(scene)


def rotated(world, degrees):
    """lookfrom turned about the vertical axis through lookat."""
    a = math.radians(degrees)
    dx, dy, dz = (f - t for f, t in zip(world.lookfrom, world.lookat))
    return (world.lookat[0] + dx * math.cos(a) + dz * math.sin(a), world.lookat[1] + dy, world.lookat[2] - dx * math.sin(a) + dz * math.cos(a))


def cameras(world, w, h):
    """The scene's own camera, two turned by +-30 degrees with another field of view, one with aperture 0.1, one with the
    shutter open from 0.25 to 0.75."""
    up, asp = (0, 1, 0), w / h
    return [art.camera(world.lookfrom, world.lookat, up, world.vfov, asp, world.aperture, 10.0, 0.0, 1.0),
            art.camera(rotated(world, 30.0), world.lookat, up, world.vfov * 1.25, asp, world.aperture, 10.0, 0.0, 1.0),
            art.camera(rotated(world, -30.0), world.lookat, up, world.vfov * 0.75, asp, world.aperture, 10.0, 0.0, 1.0),
            art.camera(world.lookfrom, world.lookat, up, world.vfov, asp, 0.1, 10.0, 0.0, 1.0),
            art.camera(world.lookfrom, world.lookat, up, world.vfov, asp, world.aperture, 10.0, 0.25, 0.75)]


def render_one(world, cam, w, h, spp, seed, max_depth=50, global_scene=False):
    """engine.run of one view: (rgb, sums, stats)."""
    eng = art.engine(cam, art.engine_mode.single, width=w, height=h, samples_per_pixel=spp, seed=seed, max_depth=max_depth)
    eng.global_scene = global_scene
    eng.set_scene(world.objects, world.background)
    img, acc = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.float64)
    eng.run(img, accum=acc)
    return img, acc, eng.stats


@functools.lru_cache(maxsize=None)
def reference(scene, global_scene=False):
    """The five views of `scene` at W x H x SPP with seeds 3 + v through engine.run, computed once and read-only."""
    world = world_of(scene)
    runs = [render_one(world, cam, W, H, SPP, SEED0 + v, global_scene=global_scene) for v, cam in enumerate(cameras(world, W, H))]
    rgb, acc = np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs])
    rgb.setflags(write=False)
    acc.setflags(write=False)
    return rgb, acc, sum(r[2]["segments"] for r in runs), sum(r[2]["primary"] for r in runs)


# ------------------------------------------------------------------------------------------------ 1. equality with rt_render
@pytest.mark.parametrize("scene,global_scene", [("1", False), ("1", True), ("4", False), ("8", False), ("cow", False), ("9", False)])
def test_every_view_equals_the_render_of_its_camera_and_seed(gpu, scene, global_scene):
    world = world_of(scene)
    rgb, acc, segments, primary = reference(scene, global_scene)
    got, sums, st = art.render_views(world, cameras(world, W, H), W, H, SPP, seeds=[SEED0 + v for v in range(5)], global_scene=global_scene,
                                     accum=True, stats=True)
    assert got.shape == (5, H, W, 3) and got.dtype == np.uint8 and sums.shape == (5, H, W, 3) and sums.dtype == np.float64
    for v in range(5):
        assert (bits(sums[v]) == bits(acc[v])).all(), (v, int((bits(sums[v]) != bits(acc[v])).sum()))
        assert (got[v] == rgb[v]).all(), v
        assert got[v].max() > 0  # no frame is black
    assert st["segments"] == segments and st["primary"] == primary == 5 * W * H * SPP
    assert st["passes"] == 1 and st["ms"] > 0


# ------------------------------------------------------------------------------------------------ 2. one seed for every view
def test_without_seeds_every_view_takes_the_params_seed(gpu):
    world = world_of("1")
    cams = cameras(world, W, H)
    got, sums = art.render_views(world, cams, W, H, SPP, seed=11, accum=True)
    for v, cam in enumerate(cams):
        img, acc, _ = render_one(world, cam, W, H, SPP, 11)
        assert (bits(sums[v]) == bits(acc)).all() and (got[v] == img).all(), v
    one, one_sums, st = art.render_views(world, cams[1:2], W, H, SPP, seed=11, accum=True, stats=True)
    assert one.shape == (1, H, W, 3) and (one[0] == got[1]).all() and (bits(one_sums[0]) == bits(sums[1])).all()
    assert st["primary"] == W * H * SPP


# ------------------------------------------------------------------------------------------------ 3. every lane refills
@pytest.mark.parametrize("scene,global_scene", [("1", False), ("1", True), ("8", False), ("cow", False)])
def test_nine_views_of_ten_grids_of_paths_on_device_tensors(gpu, scene, global_scene):
    # 9 x 128 x 72 x 32 = 2 654 208 paths against the 262 144 lanes of a full persistent grid: every lane starts ~10 paths
    import torch
    w, h, k, nv = 128, 72, 32, 9
    world = world_of(scene)
    cams = [art.camera(rotated(world, 8.0 * (v - 4)), world.lookat, (0, 1, 0), world.vfov, w / h, world.aperture, 10.0, 0.0, 1.0) for v in range(nv)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        want_rgb = torch.zeros((nv, h, w, 3), dtype=torch.uint8, device="cuda")
        want_acc = torch.zeros((nv, h, w, 3), dtype=torch.float64, device="cuda")
        segments = 0
        for v, cam in enumerate(cams):
            eng = art.engine(cam, art.engine_mode.single, width=w, height=h, samples_per_pixel=k, seed=20 + v)
            eng.global_scene = global_scene
            eng.set_scene(world.objects, world.background)
            eng.run(want_rgb[v], accum=want_acc[v], stream=side.cuda_stream)
            segments += eng.stats["segments"]
        out = torch.full((nv, h, w, 3), 7, dtype=torch.uint8, device="cuda")
        acc = torch.full((nv, h, w, 3), 7.0, dtype=torch.float64, device="cuda")
        got, sums, st = art.render_views(world, cams, w, h, k, seeds=[20 + v for v in range(nv)], global_scene=global_scene, accum=acc, out=out,
                                         stats=True)
    assert got is out and sums is acc
    side.synchronize()
    assert torch.equal(acc.view(torch.int64), want_acc.view(torch.int64))
    assert torch.equal(out, want_rgb)
    assert st["segments"] == segments and st["primary"] == nv * w * h * k and st["passes"] == 1


# ------------------------------------------------------------------------------------------------ 4. groups
def test_views_cut_into_three_launches_give_the_same_frames(gpu, options):
    world = world_of("cow")
    cams, seeds = cameras(world, W, H), [SEED0 + v for v in range(5)]
    rgb, acc, segments, _ = reference("cow")
    options("views.max_paths", 2 * W * H * SPP)  # two views a launch: 2 + 2 + 1
    got, sums, st = art.render_views(world, cams, W, H, SPP, seeds=seeds, accum=True, stats=True)
    options("views.max_paths", 0)
    assert st["passes"] == 3
    assert (got == rgb).all() and (bits(sums) == bits(acc)).all() and st["segments"] == segments
    whole, whole_sums, st1 = art.render_views(world, cams, W, H, SPP, seeds=seeds, accum=True, stats=True)
    assert st1["passes"] == 1 and (whole == got).all() and (bits(whole_sums) == bits(sums)).all()


# ------------------------------------------------------------------------------------------------ 5. one sample, depth one
@pytest.mark.parametrize("scene", ["1", "cow"])
def test_one_sample_per_pixel_has_no_sample_sum(gpu, scene):
    world = world_of(scene)
    cams = cameras(world, W, H)
    got, sums, st = art.render_views(world, cams, W, H, 1, seeds=[SEED0 + v for v in range(5)], accum=True, stats=True)
    segments = 0
    for v, cam in enumerate(cams):
        img, acc, s = render_one(world, cam, W, H, 1, SEED0 + v)
        assert (bits(sums[v]) == bits(acc)).all() and (got[v] == img).all(), v
        segments += s["segments"]
    assert st["segments"] == segments and sums.max() > 0.0


@pytest.mark.parametrize("scene", ["1", "cow"])
def test_depth_one_equals_the_render_at_depth_one(gpu, scene):
    world = world_of(scene)
    cams = cameras(world, W, H)
    got, sums, st = art.render_views(world, cams, W, H, SPP, max_depth=1, seeds=[SEED0 + v for v in range(5)], accum=True, stats=True)
    for v, cam in enumerate(cams):
        img, acc, _ = render_one(world, cam, W, H, SPP, SEED0 + v, max_depth=1)
        assert (bits(sums[v]) == bits(acc)).all() and (got[v] == img).all(), v
    assert st["segments"] == st["primary"] == 5 * W * H * SPP  # one segment a path


# ------------------------------------------------------------------------------------------------ 6. host and device buffers
@pytest.mark.parametrize("scene", ["1", "cow"])
def test_host_and_device_buffers_agree(gpu, scene):
    import torch
    world = world_of(scene)
    rgb, acc, segments, _ = reference(scene)
    cams, seeds = cameras(world, W, H), [SEED0 + v for v in range(5)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = torch.full((5, H, W, 3), 7, dtype=torch.uint8, device="cuda")
        sums = torch.full((5, H, W, 3), 7.0, dtype=torch.float64, device="cuda")
        got = art.render_views(world, cams, W, H, SPP, seeds=seeds, out=out)  # no stats: enqueued on `side`, not waited for
        assert got is out
        side.synchronize()
        assert (out.cpu().numpy() == rgb).all()
        out.fill_(7)
        _, got_sums, st = art.render_views(world, cams, W, H, SPP, seeds=seeds, out=out, accum=sums, stats=True)  # with stats the call waits
    assert got_sums is sums and st["segments"] == segments
    assert (out.cpu().numpy() == rgb).all() and (bits(sums.cpu().numpy()) == bits(acc)).all()
    host = np.zeros((5, H, W, 3), np.uint8)
    assert art.render_views(world, cams, W, H, SPP, seeds=seeds, out=host) is host and (host == rgb).all()


@pytest.mark.parametrize("scene", ["1", "cow"])
def test_device_buffers_on_the_null_stream_agree_with_host_buffers(gpu, scene):
    # torch's default stream has the null handle: the call runs on the scene's own stream and waits.  2 views of 16 x 16 x 2
    import torch
    world = world_of(scene)
    cams = cameras(world, 16, 16)[:2]
    host, host_sums = art.render_views(world, cams, 16, 16, 2, seeds=[5, 6], accum=True)
    assert torch.cuda.current_stream().cuda_stream == 0
    out = torch.full((2, 16, 16, 3), 7, dtype=torch.uint8, device="cuda")
    sums = torch.full((2, 16, 16, 3), 7.0, dtype=torch.float64, device="cuda")
    assert art.render_views(world, cams, 16, 16, 2, seeds=[5, 6], out=out, accum=sums)[0] is out
    assert (out.cpu().numpy() == host).all() and (bits(sums.cpu().numpy()) == bits(host_sums)).all()
    assert host.max() > 0
