"""rt_radiance_rays and rt_camera_rays on the GPU.  The composition is checked against the renderer bit for bit: engine.run's
radiance sums of a pixel equal the in-order f64 sum over its samples of radiance_rays(camera_rays(...)), and the segment
counts are equal -- on every builtin scene, under a band partition, and at a size where every lane of the persistent grid
refills several times.  Then the call's own parameters: samples per ray, stream ids, max_depth, host against device
buffers, the workspace fault point, and camera_rays alone.  Every comparison is of bit patterns."""
import functools

import numpy as np
import pytest

import another_raytracer_amd as art

pytestmark = pytest.mark.gpu

SCENES = ["c1", "1", "2", "3", "4", "5", "6", "7", "8", "cow", "dino", "9"]  # tests/test_gpu_parity.py's
W, H, SPP, SEED = 64, 36, 8, 3


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@functools.lru_cache(maxsize=None)
def world_of(scene):
    return art.scene_manager().build(scene)


def camera_of(world, w, h, aperture=None):
    return art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, w / h, world.aperture if aperture is None else aperture, 10.0, 0.0, 1.0)


def engine_of(world, w, h, spp, seed, max_depth=50):
    eng = art.engine(camera_of(world, w, h), art.engine_mode.single, width=w, height=h, samples_per_pixel=spp, seed=seed, max_depth=max_depth)
    eng.set_scene(world.objects, world.background)
    return eng


def sum_in_sample_order(L, k):
    """(pixels * k, 3) per-sample values -> (pixels, 3): 0.0 + L[., 0] + L[., 1] + ... (numpy or torch)."""
    per = L.reshape(-1, k, 3)
    if isinstance(per, np.ndarray):
        acc = np.zeros_like(per[:, 0])
    else:
        import torch
        acc = torch.zeros_like(per[:, 0])
    for s in range(k):
        acc = acc + per[:, s]
    return acc


def render_and_compose(scene, bands=None):
    world = world_of(scene)
    eng = engine_of(world, W, H, SPP, SEED)
    band_rows, band_count, band_index = bands or (None, 1, 0)
    rows = H if bands is None else len(eng.local_rows(*bands))
    img, acc = np.zeros((rows, W, 3), np.uint8), np.zeros((rows, W, 3), np.float64)
    eng.run(img, accum=acc, band_rows=band_rows, band_count=band_count, band_index=band_index)
    rays, rng = art.camera_rays(eng.cam, W, H, SPP, seed=SEED, bands=bands)
    assert rays.shape == (rows * W * SPP, 7) and rng.shape == (rows * W * SPP,) and rng.dtype == np.uint64
    L, st = art.radiance_rays(world, rays, rng=rng, spp=1, max_depth=50, stats=True)
    return acc.reshape(-1, 3), eng.stats, sum_in_sample_order(L, SPP), st


# ------------------------------------------------------------------------------------------------ 1. composition == rt_render
@pytest.mark.parametrize("scene", SCENES)
def test_radiance_of_the_camera_rays_sums_to_the_render(gpu, scene):
    acc, stats, composed, st = render_and_compose(scene)
    assert (bits(composed) == bits(acc)).all(), int((bits(composed) != bits(acc)).sum())
    assert st["segments"] == stats["segments"] and st["primary"] == W * H * SPP == stats["primary"]
    assert acc.max() > 0.0  # the frame is not black


def test_the_composition_under_a_band_partition(gpu):
    acc, stats, composed, st = render_and_compose("6", bands=(8, 2, 1))
    assert acc.shape[0] == 16 * W  # rows 8-15 and 24-31
    assert (bits(composed) == bits(acc)).all()
    assert st["segments"] == stats["segments"]


# ------------------------------------------------------------------------------------------------ 2. every lane refills
@pytest.mark.parametrize("scene,global_scene", [("1", False), ("1", True), ("8", False), ("cow", False)])
def test_a_frame_of_nine_grids_of_paths_on_device_tensors(gpu, scene, global_scene):
    # 256 x 144 x 64 = 2 359 296 paths against the 262 144 lanes of a full persistent grid: every lane starts ~9 paths
    import torch
    w, h, k = 256, 144, 64
    world = world_of(scene)
    eng = engine_of(world, w, h, k, SEED)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        img = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        acc = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
        eng.run(img, accum=acc, stream=side.cuda_stream)
        rays, rng = art.camera_rays(eng.cam, w, h, k, seed=SEED, device=0)
        assert rays.is_cuda and tuple(rays.shape) == (w * h * k, 7) and rng.dtype == torch.int64
        L, st = art.radiance_rays(world, rays, rng=rng, spp=1, global_scene=global_scene, stats=True)
        assert L.is_cuda and L.dtype == torch.float64
        composed = sum_in_sample_order(L, k)
    side.synchronize()
    assert torch.equal(composed.view(torch.int64), acc.reshape(-1, 3).view(torch.int64))
    assert st["segments"] == eng.stats["segments"] and st["primary"] == w * h * k


# ------------------------------------------------------------------------------------------------ 3.-5. the call's parameters
@functools.lru_cache(maxsize=None)
def probe_rays(scene, n=4096):
    """n of the scene's camera rays (64 x 64 pixels, one sample), read-only."""
    rays, _ = art.camera_rays(camera_of(world_of(scene), 64, 64), 64, 64, 1, seed=1)
    rays = np.ascontiguousarray(rays[:n])
    rays.setflags(write=False)
    return rays


def test_samples_per_ray_are_summed_in_sample_order(gpu):
    # 70 samples: more than a wave's 64 lanes per ray and no multiple of 64
    world, rays = world_of("6"), probe_rays("6")
    whole = art.radiance_rays(world, rays, spp=70, sample_base=5, seed=9)
    acc = np.zeros((len(rays), 3))
    for s in range(70):
        acc = acc + art.radiance_rays(world, rays, spp=1, sample_base=5 + s, seed=9)
    assert (bits(whole) == bits(acc)).all()
    assert whole.max() > 0.0


def test_stream_ids_follow_id_base_and_the_seed_matters(gpu):
    world, rays = world_of("6"), probe_rays("6")
    whole = art.radiance_rays(world, rays, spp=3, seed=9)
    a, b = 1001, 3003
    part = art.radiance_rays(world, np.ascontiguousarray(rays[a:b]), spp=3, seed=9, id_base=a)
    assert (bits(part) == bits(whole[a:b])).all()
    assert (bits(art.radiance_rays(world, rays, spp=3, seed=9)) == bits(whole)).all()
    assert (bits(art.radiance_rays(world, rays, spp=3, seed=10)) != bits(whole)).any()
    assert (bits(art.radiance_rays(world, np.ascontiguousarray(rays[a:b]), spp=3, seed=9)) != bits(whole[a:b])).any()  # id_base 0


def test_max_depth_one_returns_the_background_on_a_miss_and_nothing_else(gpu):
    world, rays = world_of("1"), probe_rays("1")
    bg = (0.25, 0.5, 0.75)
    L = art.radiance_rays(world, rays, max_depth=1, background=bg)
    miss = ~np.isfinite(art.query_rays(world.objects, rays).t)
    assert miss.any() and (~miss).any()
    assert (L[miss] == np.array(bg)).all() and (bits(L[~miss]) == 0).all()


# ------------------------------------------------------------------------------------------------ 6. host and device buffers
@pytest.mark.parametrize("scene", ["1", "cow"])
def test_host_and_device_buffers_agree(gpu, scene):
    import torch
    world, rays = world_of(scene), probe_rays(scene)
    host, st = art.radiance_rays(world, rays, spp=5, seed=2, stats=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_rays = torch.from_numpy(np.array(rays, order="C")).to("cuda")
        out = torch.full((len(rays), 3), 7.0, dtype=torch.float64, device="cuda")
        got = art.radiance_rays(world, d_rays, spp=5, seed=2, out=out)  # no stats: enqueued on `side`, not waited for
    assert got is out
    side.synchronize()
    assert (bits(out.cpu().numpy()) == bits(host)).all()
    with torch.cuda.stream(side):
        dev, dst = art.radiance_rays(world, d_rays, spp=5, seed=2, stats=True)  # with stats the call waits
    assert (bits(dev.cpu().numpy()) == bits(host)).all()
    assert dst["segments"] == st["segments"] and dst["primary"] == 5 * len(rays) and st["ms"] > 0


@pytest.mark.parametrize("scene", ["1", "cow"])
def test_device_buffers_on_the_null_stream_agree_with_host_buffers(gpu, scene):
    # torch's default stream has the null handle: the call runs on the scene's own stream and waits.  65 rays: a wave and one
    import torch
    world, rays = world_of(scene), np.array(probe_rays(scene)[:65])  # a writable copy
    host = art.radiance_rays(world, rays, spp=2, seed=3)
    assert torch.cuda.current_stream().cuda_stream == 0
    out = torch.full((65, 3), 7.0, dtype=torch.float64, device="cuda")
    got = art.radiance_rays(world, torch.from_numpy(rays).to("cuda"), spp=2, seed=3, out=out)
    assert got is out and (bits(out.cpu().numpy()) == bits(host)).all()
    assert host.max() > 0.0


def test_camera_rays_on_the_null_stream_agree_with_host_buffers(gpu):
    import torch
    cam = camera_of(world_of("1"), 13, 5)
    rays, rng = art.camera_rays(cam, 13, 5, 1, seed=7)  # 65 rays
    assert torch.cuda.current_stream().cuda_stream == 0
    d_rays, d_rng = art.camera_rays(cam, 13, 5, 1, seed=7, device=0)
    assert d_rays.is_cuda and tuple(d_rays.shape) == (65, 7)
    assert (bits(d_rays.cpu().numpy()) == bits(rays)).all() and (d_rng.cpu().numpy().view(np.uint64) == rng).all()


# ------------------------------------------------------------------------------------------------ 7. the workspace fault point
def test_a_refused_workspace_fails_the_call_and_the_next_one_works(gpu, options):
    # an injected allocation refusal on the host (test.fault_workspace_bytes), on a scene of its own: its workspace is empty
    world, rays = art.scene_manager().build("c1"), probe_rays("c1")
    want = art.radiance_rays(world_of("c1"), rays, spp=8, seed=4)
    options("test.fault_workspace_bytes", 4096)
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.radiance_rays(world, rays, spp=8, seed=4)
    options("test.fault_workspace_bytes", 0)
    assert (bits(art.radiance_rays(world, rays, spp=8, seed=4)) == bits(want)).all()


# ------------------------------------------------------------------------------------------------ 8. camera_rays alone
def test_camera_rays_alone(gpu):
    world = world_of("1")
    w, h = 40, 30
    pinhole = camera_of(world, w, h, aperture=0.0)
    rays, rng = art.camera_rays(pinhole, w, h, 5, seed=7)
    assert (rays[:, 0:3] == np.array(world.lookfrom, np.float64)).all()  # no lens offset: every origin is lookfrom
    assert ((rays[:, 6] >= 0.0) & (rays[:, 6] <= 1.0)).all() and len(np.unique(rng)) == len(rng)
    cam = camera_of(world, w, h)
    assert world.aperture > 0
    rays, rng = art.camera_rays(cam, w, h, 5, seed=7)
    again = art.camera_rays(cam, w, h, 5, seed=7)
    assert (bits(rays) == bits(again[0])).all() and (rng == again[1]).all()
    tail = art.camera_rays(cam, w, h, 2, seed=7, sample_base=3)
    assert (bits(rays.reshape(-1, 5, 7)[:, 3:5]) == bits(tail[0].reshape(-1, 2, 7))).all()
    assert (rng.reshape(-1, 5)[:, 3:5] == tail[1].reshape(-1, 2)).all()
    assert (bits(rays[:, 0:3]) != bits(np.broadcast_to(np.array(world.lookfrom, np.float64), (len(rays), 3)))).any()  # the lens
