"""rt_query_rays on the GPU: the closest hit equals rt_trace_rays bit for bit and carries the whole hit_record; RT_Q_NO_MEDIA
gives the closest surface; the any-hit query equals the closest search for every ray, whatever the tree, the child order,
LDS or HBM; device tensors on a caller's stream give the host path's results.

Rays: tests.test_gpu_rays.ray_sets (camera-like rays, continuations from surfaces, axis-parallel and tiny-component rays,
5 374 - 14 644 per scene, no length a multiple of 256); the CPU oracle has no NaN closest hit among them, so every ray takes
part in every comparison.  Each scene's rays and references are computed once and shared (read-only)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import check, lib, rt_scene_info
from tests.oracle_lib import oracle_trace_rays
from tests.test_gpu_guides import frame
from tests.test_gpu_rays import SCENES, gpu_trace, ray_sets

pytestmark = pytest.mark.gpu

# scenes with a constant_medium (rt_scene_info.has_media): the Cornell smoke, the Next-Week final, and the three mesh scenes,
# whose meshes stand in a fog sphere; test_no_media_... asserts the split, so all 11 scenes are in one class or the other
MEDIA_SCENES = ["7", "8", "cow", "dino", "9"]
MEDIA_FREE = [s for s in SCENES if s not in MEDIA_SCENES]
T, NRM, PNT, U, V, FF, PRIM, MAT = 0, slice(1, 4), slice(4, 7), 7, 8, 9, 10, 11
MISS = [math.inf, 0, 0, 0, math.inf, math.inf, math.inf, 0, 0, 0, -1, -1]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    # any NaN equals any NaN, as tests/test_gpu_rays.py compares (x86 and gfx950 give 0/0 different sign bits)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def world_of(scene):
    return art.scene_manager().build(scene)


@functools.lru_cache(maxsize=None)
def rays_of(scene):
    return frozen(np.ascontiguousarray(ray_sets(scene)))


@functools.lru_cache(maxsize=None)
def trace_of(scene, global_scene=False):
    """rt_trace_rays of the scene's rays: (t, normal)."""
    t, nrm, _ = gpu_trace(scene, rays_of(scene), global_scene)
    return frozen(t, nrm)


@functools.lru_cache(maxsize=None)
def closest_of(scene, no_media=False):
    """The (n, 12) records of the scene's rays through host buffers."""
    return frozen(art.query_rays(world_of(scene).objects, rays_of(scene), no_media=no_media).records)


def on_device(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda")  # a copy: the shared arrays are read-only


def materials_of(handle):
    info = rt_scene_info()
    check(lib.rt_scene_info_get(handle, ctypes.byref(info)), "rt_scene_info_get")
    return int(info.materials)


# ------------------------------------------------------------------------------------------------ 1. closest == rt_trace_rays
@pytest.mark.parametrize("scene", SCENES)
def test_closest_mode_equals_trace_rays_on_host_and_device_buffers(gpu, scene):
    rays = rays_of(scene)
    assert len(rays) % 256 != 0
    t, nrm = trace_of(scene)
    host = closest_of(scene)
    assert same_bits(host[:, T], t).all() and same_bits(host[:, NRM], nrm).all()
    dev = art.query_rays(world_of(scene).objects, on_device(rays))
    assert dev.records.is_cuda and tuple(dev.records.shape) == (len(rays), 12)
    assert same_bits(dev.records.cpu().numpy(), host).all()  # every column, not only t and the normal


@pytest.mark.parametrize("global_scene", [False, True])
def test_lds_and_hbm_traversals_give_the_same_records(gpu, global_scene):
    t, nrm = trace_of("1", global_scene)
    rec = art.query_rays(world_of("1").objects, rays_of("1"), global_scene=global_scene).records
    assert same_bits(rec[:, T], t).all() and same_bits(rec[:, NRM], nrm).all()
    assert same_bits(rec, closest_of("1")).all()


@pytest.mark.parametrize("scene", ["1", "8"])
@pytest.mark.parametrize("n", [1, 63, 1025])
def test_small_and_odd_ray_counts(gpu, scene, n):
    # less than a wave, less than a block, one lane past a 1024-lane block; ray i keeps its medium stream i
    rays = np.ascontiguousarray(rays_of(scene)[:n])
    t, nrm, _ = gpu_trace(scene, rays)
    rec = art.query_rays(world_of(scene).objects, rays).records
    assert rec.shape == (n, 12)
    assert same_bits(rec[:, T], t).all() and same_bits(rec[:, NRM], nrm).all()
    assert same_bits(rec, closest_of(scene)[:n]).all()
    out = np.full((n + 1, 12), 7.0)  # the call writes n records and nothing behind them
    art.query_rays(world_of(scene).objects, rays, out=out[:n])
    assert same_bits(out[:n], rec).all() and (out[n] == 7.0).all()


# ------------------------------------------------------------------------------------------------ 2. the record's fields
@pytest.mark.parametrize("scene", ["1", "6", "8", "cow"])
def test_point_normal_and_t_equal_the_guide_buffers(gpu, scene):
    # the guides' rays with the same ray index, and so the same medium streams
    W, H = 64, 36
    world, _, guides, rays = frame(scene, W, H)
    rec = art.query_rays(world.objects, np.ascontiguousarray(rays.reshape(-1, 7))).records
    g = guides.reshape(-1, 10)
    assert same_bits(rec[:, T], g[:, 9]).all()
    assert same_bits(rec[:, NRM], g[:, 3:6]).all()
    assert same_bits(rec[:, PNT], g[:, 6:9]).all()
    hit = np.isfinite(rec[:, T])
    assert hit.any() and ((rec[hit, FF] == 0.0) | (rec[hit, FF] == 1.0)).all()
    mats = materials_of(world.objects._native)
    assert ((rec[hit, MAT] >= 0) & (rec[hit, MAT] < mats) & (rec[hit, MAT] == np.floor(rec[hit, MAT]))).all()
    assert (rec[~hit] == np.array(MISS)).all()


SPHERES = [((-3.0, 1.0, 0.0), 1.0), ((0.0, 1.0, 0.0), 0.8), ((3.0, 1.0, 0.5), 1.0)]
RECT = (-2.0, 2.0, -1.0, 1.5, 4.0)  # x0, x1, z0, z1, y
BOX_AT = (6.0, 0.0, -1.0)


@functools.lru_cache(maxsize=None)
def graph_scene():
    """Three disjoint spheres with three materials, one xz_rect, one box under translate(rotate_y): five materials."""
    art.reset_scene_rng()
    world = art.hittable_list()
    for (c, r), m in zip(SPHERES, (art.lambertian((0.8, 0.1, 0.15)), art.metal((0.6, 0.55, 0.4), 0.1), art.dielectric(1.5))):
        world.add(art.sphere(c, r, m))
    world.add(art.xz_rect(*RECT, art.diffuse_light((7.0, 6.0, 5.0))))
    world.add(art.translate(art.rotate_y(art.box((0.0, 0.0, 0.0), (1.0, 2.0, 1.0), art.lambertian((0.73, 0.73, 0.73))), 20.0), BOX_AT))
    handle = art.compile_world(world, 0)
    art.reset_scene_rng()
    return handle


def rays_towards(rng, origin, target, spread, n):
    o = np.tile(np.array(origin, float), (n, 1))
    d = (np.array(target, float) + rng.uniform(-1.0, 1.0, (n, 3)) * np.array(spread, float)) - o
    return np.column_stack([o, d, rng.random(n)])


def test_prim_mat_front_face_and_uv_on_a_graph_scene(gpu):
    h = graph_scene()
    rng = np.random.default_rng(3)
    eye = (0.5, 2.0, 14.0)
    groups = [rays_towards(rng, eye, c, 0.5 * r, 301) for c, r in SPHERES]
    groups.append(rays_towards(rng, (0.0, 2.5, 0.2), (0.0, RECT[4], 0.25), (1.5, 0.0, 0.9), 301))  # up at the rect from below
    # the box's centre (0.5, 1, 0.5) turned by 20 degrees about y and moved by BOX_AT
    groups.append(rays_towards(rng, eye, (BOX_AT[0] + 0.641, 1.0, BOX_AT[2] + 0.299), 0.2, 301))
    rays = np.concatenate(groups)
    rec = art.query_rays(h, rays).records
    owner = np.repeat(np.arange(5), 301)
    assert np.isfinite(rec[:, T]).all()
    # the hit is on the object aimed at
    for k, (c, r) in enumerate(SPHERES):
        assert (np.abs(np.linalg.norm(rec[owner == k, PNT] - np.array(c), axis=1) - r) <= 1e-9).all(), k
    assert (np.abs(rec[owner == 3, 5] - RECT[4]) <= 1e-12).all()
    # prim: one value per object, five different ones; mat: as many values as the scene has materials
    prims = [np.unique(rec[owner == k, PRIM]) for k in range(5)]
    assert all(len(p) == 1 and p[0] >= 0 and p[0] == np.floor(p[0]) for p in prims), prims
    assert len({float(p[0]) for p in prims}) == 5
    mats = materials_of(h)
    assert mats == 5
    assert sorted(np.unique(rec[:, MAT]).tolist()) == list(range(mats))
    assert all(len(np.unique(rec[owner == k, MAT])) == 1 for k in range(5))
    # front_face: 1 from outside a sphere, 0 from its centre (and the normal then points back at the centre)
    assert (rec[owner < 3, FF] == 1.0).all()
    for c, r in SPHERES:
        d = rng.normal(0, 1, (101, 3))
        inside = art.query_rays(h, np.column_stack([np.tile(np.array(c), (101, 1)), d, np.zeros(101)])).records
        assert (inside[:, FF] == 0.0).all() and np.isfinite(inside[:, T]).all()
        assert (np.einsum("ij,ij->i", inside[:, NRM], d) < 0).all()
    # rect u, v: exactly aarect.cpp:29-30 on the record's own point
    x0, x1, z0, z1, _ = RECT
    on_rect = rec[owner == 3]
    assert (on_rect[:, U] == (on_rect[:, 4] - x0) / (x1 - x0)).all() and (on_rect[:, V] == (on_rect[:, 6] - z0) / (z1 - z0)).all()
    assert ((on_rect[:, U] > 0) & (on_rect[:, U] < 1)).all() and len(np.unique(on_rect[:, U])) > 100
    # sphere u, v: get_sphere_uv (sphere.h:24-37) of the outward normal (p - c) / r = (1 / r) * (p - c), with the C
    # library's acos / atan2 (Python's math module calls them): the product restates glibc's, so <= 1e-12 covers a libm
    # whose last bit differs from glibc 2.35's
    for k, (c, r) in enumerate(SPHERES):
        s = rec[owner == k]
        n = (1.0 / r) * (s[:, PNT] - np.array(c))
        u = np.array([(math.atan2(-z, x) + math.pi) / (2 * math.pi) for x, _, z in n])
        v = np.array([math.acos(-y) / math.pi for _, y, _ in n])
        assert np.abs(s[:, U] - u).max() <= 1e-12 and np.abs(s[:, V] - v).max() <= 1e-12, k
        assert len(np.unique(s[:, U])) > 100
    # each side of the box sets the rect's u, v
    on_box = rec[owner == 4]
    assert ((on_box[:, U] >= 0) & (on_box[:, U] <= 1) & (on_box[:, V] >= 0) & (on_box[:, V] <= 1)).all() and (on_box[:, U] != 0).any()


def test_a_miss_has_the_documented_record(gpu):
    h = graph_scene()
    # (off y = 0: a ray with d.y = 0 in the plane of the box's bottom side has t = 0/0 there, which aarect.cpp accepts)
    away = np.array([[0.0, 10.0, 0.0, 0.0, 1.0, 0.0, 0.5], [50.0, 0.3, 0.2, 1.0, 0.0, 0.0, 0.0], [0.5, 2.0, 14.0, 0.1, 0.2, 1.0, 0.25]])
    rec = art.query_rays(h, away).records
    assert (rec == np.array(MISS)).all()
    # and a hit beyond t_max is a miss: the same rays towards the scene with t_max in front of it
    rays = rays_towards(np.random.default_rng(5), (0.5, 2.0, 14.0), SPHERES[1][0], 0.3, 65)
    full = art.query_rays(h, rays).records
    assert np.isfinite(full[:, T]).all()
    cut = art.query_rays(h, rays, t_max=0.5 * np.ascontiguousarray(full[:, T])).records
    assert (cut == np.array(MISS)).all()
    keep = art.query_rays(h, rays, t_max=np.ascontiguousarray(full[:, T]) * (1 + 2.0 ** -20)).records
    assert same_bits(keep, full).all()


# ------------------------------------------------------------------------------------------------ 3. RT_Q_NO_MEDIA
@pytest.mark.parametrize("scene", MEDIA_FREE)
def test_no_media_changes_nothing_without_media(gpu, scene):
    assert world_of(scene).info["has_media"] == 0
    assert same_bits(closest_of(scene, no_media=True), closest_of(scene)).all()


def media_scene(with_media):
    """Spheres, a rect and a box, with a constant_medium over a sphere boundary and one over a box boundary between them
    in the world list (scene A) or without the two media (scene B)."""
    art.reset_scene_rng()
    grey, red = art.lambertian((0.7, 0.7, 0.7)), art.lambertian((0.8, 0.1, 0.1))
    world = art.hittable_list()
    world.add(art.sphere((-3.0, 1.0, 0.0), 1.0, red))
    if with_media:
        world.add(art.constant_medium(art.sphere((0.0, 1.5, 1.0), 1.5, art.dielectric(1.5)), 0.6, (1.0, 1.0, 1.0)))
    world.add(art.sphere((3.0, 1.0, -0.5), 1.0, art.metal((0.6, 0.55, 0.4), 0.0)))
    world.add(art.xz_rect(-8.0, 8.0, -8.0, 8.0, 0.0, grey))
    if with_media:
        world.add(art.constant_medium(art.translate(art.rotate_y(art.box((0.0, 0.0, 0.0), (2.0, 2.0, 2.0), grey), 15.0), (1.0, 0.0, -4.0)),
                                      0.4, (0.2, 0.2, 0.2)))
    world.add(art.translate(art.rotate_y(art.box((0.0, 0.0, 0.0), (1.0, 2.5, 1.0), grey), -25.0), (-1.5, 0.0, -3.0)))
    world.add(art.sphere((0.5, 0.6, 3.0), 0.6, art.dielectric(1.5)))
    handle = art.compile_world(world, 0)
    art.reset_scene_rng()
    return handle


def test_no_media_equals_the_scene_without_its_media(gpu):
    a, b = media_scene(True), media_scene(False)
    rng = np.random.default_rng(17)
    n = 4099
    o = np.array([0.0, 3.0, 11.0]) + rng.normal(0, 0.3, (n, 3))
    d = (np.array([0.0, 1.0, 0.0]) + rng.normal(0, 2.5, (n, 3))) - o
    rays = np.column_stack([o, d, rng.random(n)])
    # continuations from the first hits, many of them starting inside a medium
    first = art.query_rays(b, rays).records
    ok = np.isfinite(first[:, T])
    rays = np.concatenate([rays, np.column_stack([first[ok, PNT], rng.normal(0, 1, (ok.sum(), 3)), rng.random(ok.sum())])])
    with_media = art.query_rays(a, rays).records
    skipped = art.query_rays(a, rays, no_media=True).records
    plain = art.query_rays(b, rays).records
    for cols in (T, NRM, PNT):
        assert same_bits(skipped[:, cols], plain[:, cols]).all()
    assert same_bits(skipped[:, [U, V, FF]], plain[:, [U, V, FF]]).all()
    # the media are there: scattering events (prim -2, one isotropic material per medium) in front of the surfaces
    ev = with_media[:, PRIM] == -2.0
    assert ev.sum() > 100 and (skipped[:, PRIM] != -2.0).all()
    assert (with_media[ev, T] <= skipped[ev, T]).all() and (with_media[ev, T] < skipped[ev, T]).any()
    mats = materials_of(a)
    assert len(np.unique(with_media[ev, MAT])) == 2 and ((with_media[ev, MAT] >= 0) & (with_media[ev, MAT] < mats)).all()
    assert (with_media[ev, U] == 0).all() and (with_media[ev, V] == 0).all() and (with_media[ev, FF] == 1.0).all()
    # the same through device buffers
    dev = art.query_rays(a, on_device(rays), no_media=True).records.cpu().numpy()
    assert same_bits(dev, skipped).all()


@pytest.mark.parametrize("scene", MEDIA_SCENES)
def test_no_media_hits_are_never_nearer_than_the_reference(gpu, scene):
    assert world_of(scene).info["has_media"] == 1
    t_o, _ = oracle_trace_rays(scene, rays_of(scene))
    assert not np.isnan(t_o).any()
    t = closest_of(scene, no_media=True)[:, T]
    assert (t >= t_o).all()
    assert (closest_of(scene)[:, PRIM] == -2.0).any() and (closest_of(scene, no_media=True)[:, PRIM] >= 0).sum() > 0
    assert (t > t_o).any()


# ------------------------------------------------------------------------------------------------ 4. any hit == closest search
def t_max_vectors(t_c, seed):
    up = t_c * (1 + 2.0 ** -20)          # inf where missed
    return {"null": None, "just_behind": up, "just_in_front": t_c * (1 - 2.0 ** -20), "half": 0.5 * t_c,
            "below_t_min": np.full(len(t_c), 0.0005), "log_uniform": 10.0 ** np.random.default_rng(seed).uniform(-3, 4, len(t_c))}


def expected_occlusion(t_c, t_max):
    # the 2^-20 offsets stay clear of each primitive's own boundary rule, and below the boxes' 2e-6 padding
    return np.isfinite(t_c) & (t_c < (np.inf if t_max is None else t_max))


def check_any_hit(scene, global_scene=False):
    world, rays = world_of(scene), rays_of(scene)
    t_c = np.ascontiguousarray(closest_of(scene, no_media=True)[:, T])
    assert not np.isnan(t_c).any()
    d_rays = on_device(rays)
    try:
        for sort in (1, 0):
            art.set_option("query.any_sorted", sort)
            for name, t_max in t_max_vectors(t_c, 23).items():
                want = expected_occlusion(t_c, t_max)
                host = art.query_rays(world.objects, rays, t_max=t_max, any_hit=True, global_scene=global_scene)
                assert host.dtype == np.uint8 and host.shape == (len(rays),)
                bad = np.flatnonzero(host != want)
                assert len(bad) == 0, (scene, name, sort, len(bad), rays[bad[0]].tolist(), t_c[bad[0]], None if t_max is None else t_max[bad[0]])
                dev = art.query_rays(world.objects, d_rays, t_max=None if t_max is None else on_device(t_max), any_hit=True,
                                     global_scene=global_scene)
                assert (dev.cpu().numpy() == want).all(), (scene, name, sort, "device buffers")
                if name == "below_t_min":
                    assert not want.any()
                if name in ("null", "just_behind"):
                    assert (want == np.isfinite(t_c)).all() and want.any()
    finally:
        art.set_option(None, 0)  # every option back at its default


@pytest.mark.parametrize("scene", SCENES)
def test_any_hit_equals_the_closest_search(gpu, scene):
    check_any_hit(scene)


def test_any_hit_through_the_hbm_traversal_of_the_lds_scene(gpu):
    check_any_hit("1", global_scene=True)


def test_any_hit_writes_bool_outputs_and_only_its_own_bytes(gpu):
    world, rays = world_of("6"), np.ascontiguousarray(rays_of("6")[:1025])
    want = art.query_rays(world.objects, rays, any_hit=True)
    out = np.full(1026, 7, np.uint8)
    art.query_rays(world.objects, rays, any_hit=True, out=out[:1025])
    assert (out[:1025] == want).all() and out[1025] == 7
    flags = np.zeros(1025, bool)
    art.query_rays(world.objects, rays, any_hit=True, out=flags)
    assert (flags == want.astype(bool)).all() and want.any() and not want.all()


# ------------------------------------------------------------------------------------------------ 5. streams
@pytest.mark.parametrize("scene", ["1", "8"])
def test_a_callers_stream_gives_the_host_results(gpu, scene):
    import torch
    world, rays = world_of(scene), rays_of(scene)
    host = closest_of(scene)
    t_max = np.ascontiguousarray(0.75 * closest_of(scene, no_media=True)[:, T])
    occ_host = art.query_rays(world.objects, rays, t_max=t_max, any_hit=True)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        d_rays = torch.from_numpy(np.array(rays)).to("cuda", non_blocking=True)
        d_tmax = torch.from_numpy(np.array(t_max)).to("cuda", non_blocking=True)
        rec = art.query_rays(world.objects, d_rays)                       # torch's current stream: `side`
        occ = art.query_rays(world.objects, d_rays, t_max=d_tmax, any_hit=True, stream=side)
        twice = rec.t * 2.0                                               # ordered after the query on the same stream
    side.synchronize()
    assert same_bits(rec.records.cpu().numpy(), host).all()
    assert (occ.cpu().numpy() == occ_host).all()
    assert same_bits(twice.cpu().numpy(), 2.0 * host[:, T]).all()
