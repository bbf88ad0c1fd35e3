"""rt_scene_update_triangles on the GPU.  A scene compiled from triangles P0 and updated to P1 must give, bit for bit,
what a scene compiled fresh from P1 gives -- frames, f64 sums, segment counts, hit records, occlusion bytes -- on every
kernel family a mesh can run: the whole BVH in LDS (grid), its top levels in LDS (cow), pair-aligned leaves (capsule) and
a split BVH's duplicated references (dino).  Equality alone would pass a refit to infinite boxes and, where the mesh
only grows, one that keeps stale boxes: rays toward a mesh moved far away (they must hit it, and miss where it was) and a
numpy restatement of every box of the refitted tree rule those out.  Frames are 64 x 36 x 8, queries 4096 rays."""
import functools

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import lib
from tests.update_common import ASSETS, F_LEAF2, H, NQ, SKY, SPP, W, bits, conservative_box_np, grid_triangles, render, same_queries, same_render

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ meshes and worlds
@functools.lru_cache(maxsize=None)
def mesh(name):
    """P0 of a mesh, read-only: the grid, or the triangles of a builtin scene as scene_triangles gives them."""
    p = grid_triangles() if name == "grid" else art.scene_triangles(art.scene_manager().build({"capsule": "9"}.get(name, name)))
    p.setflags(write=False)
    return p


def box_of(p):
    lo, hi = p.reshape(-1, 3).min(0), p.reshape(-1, 3).max(0)
    return lo, hi, 0.5 * (lo + hi), float((hi - lo).max())


def twist(p):
    """A 90 degree twist about the vertical axis through the box centre, growing with height, then a 1.5 x stretch in x
    about that centre: boxes move and grow."""
    lo, hi, c, _ = box_of(p)
    q = p - c
    a = 0.5 * np.pi * (p[..., 1] - lo[1]) / (hi[1] - lo[1])
    x = np.cos(a) * q[..., 0] + np.sin(a) * q[..., 2]
    z = -np.sin(a) * q[..., 0] + np.cos(a) * q[..., 2]
    return np.ascontiguousarray(np.stack([1.5 * x, q[..., 1], z], -1) + c)


def build(p, p_frame, floor=None):
    """A world of the triangles p in a bvh_node (one solid lambertian per colour class, triangle i takes class i % 3), a
    sphere light above and a metal sphere beside the box of p_frame -- the same for every world of one test, so that the
    same call sequence gives the same material ids -- and, with `floor`, two loose triangles after the mesh.  Returns
    the compiled world as a hittable_list that engines, queries and updates take."""
    art.reset_scene_rng()
    mats = [art.lambertian(c) for c in ((0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.3, 0.3, 0.8))]
    light, mirror = art.diffuse_light((4.0, 4.0, 4.0)), art.metal((0.8, 0.8, 0.8), 0.0)
    lo, hi, c, ext = box_of(p_frame)
    w = art.hittable_list()
    w.add(art.bvh_node([art.triangle(t[0], t[1], t[2], mats[i % 3]) for i, t in enumerate(p)]))
    if floor is not None:
        grey = art.lambertian((0.5, 0.5, 0.5))
        for t in floor:
            w.add(art.triangle(t[0], t[1], t[2], grey))
    w.add(art.sphere((c[0], hi[1] + 2.0 * ext, c[2]), 0.5 * ext, light))
    w.add(art.sphere((lo[0] - ext, c[1], c[2]), 0.4 * ext, mirror))
    return art.hittable_list(native=art.compile_world(w, 0))


def frame_camera(p_frame):
    lo, hi, c, ext = box_of(p_frame)
    return art.camera((c[0] + 0.4 * ext, c[1] + 0.9 * ext, c[2] + 2.2 * ext), tuple(c), (0, 1, 0), 40.0, W / H, 0.0, 10.0, 0.0, 1.0)


def kernel_of(stats):
    return stats["kernel_features"], stats["kernel_textures"], stats["kernel_lds_mode"]


def rays_toward(p, origin, step):
    """Rays from `origin` toward the centroid of every step-th triangle of p that has an area and does not graze the ray:
    certain hits (of that triangle, or of something in front of it)."""
    origin = np.asarray(origin, np.float64)
    cen = p.mean(1)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    d = cen - origin
    size = box_of(p)[3]
    ok = (np.linalg.norm(n, axis=1) > 1e-9 * size * size) & (np.abs((n * d).sum(1)) > 1e-2 * np.linalg.norm(n, axis=1) * np.linalg.norm(d, axis=1))
    d = d[ok][::step]
    rays = np.zeros((len(d), 7))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = origin, d, 0.5
    return rays


def random_rays(p, seed=11):
    lo, hi, c, ext = box_of(p)
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(NQ, 3))
    o = c + 3.0 * ext * o / np.linalg.norm(o, axis=1, keepdims=True)
    target = rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, (NQ, 3))
    rays = np.zeros((NQ, 7))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, target - o, rng.uniform(0, 1, NQ)
    return rays


EXPECT = {"grid": lambda k, w: k[2] == 1, "cow": lambda k, w: k[2] == 2, "capsule": lambda k, w: k[0] & F_LEAF2,
          "dino": lambda k, w: len(art.scene_bvh(w)[1]) > lib.rt_scene_triangles_get(w._native, None, 0) + 2}


@functools.lru_cache(maxsize=None)
def updated_pair(name):
    """Case 1's worlds of a mesh: A = build(P0) rendered, then updated to P1 from a host array; B = build(P1).  Shared by
    the tests that only read them."""
    p0 = mesh(name)
    p1 = twist(p0)
    a = build(p0, p1)
    cam = frame_camera(p1)
    before = render(a, cam)
    bvh_before = art.scene_bvh(a)
    art.update_triangles(a, p1)
    b = build(p1, p1)
    return a, b, p1, cam, before, bvh_before


# ------------------------------------------------------------------------------------------------ 1. equality with a fresh compile
@pytest.mark.parametrize("name", ["grid", "cow", "capsule", "dino"])
def test_an_updated_scene_equals_the_fresh_compile_of_its_vertices(gpu, name):
    a, b, p1, cam, before, _ = updated_pair(name)
    ra, rb = render(a, cam), render(b, cam)
    assert EXPECT[name](kernel_of(ra[2]), a), (name, kernel_of(ra[2]))  # the kernel family this case is here for
    assert kernel_of(ra[2]) == kernel_of(before[2]) and ra[2]["extend_variant"] == before[2]["extend_variant"] == 4
    assert same_render(ra, rb), (int((ra[0] != rb[0]).sum()), ra[2]["segments"], rb[2]["segments"])
    assert not same_render(ra, before) and ra[0].max() > 0  # the update is visible
    assert (bits(art.scene_triangles(a)) == bits(p1)).all()
    lo, hi, c, ext = box_of(p1)
    cam_rays, _ = art.camera_rays(cam, W, H, 2)
    same_queries(a, b, np.ascontiguousarray(cam_rays[:NQ]))
    hits = same_queries(a, b, rays_toward(p1, (c[0], c[1] + 0.5 * ext, c[2] + 4.0 * ext), max(1, len(p1) // NQ)))
    assert np.isfinite(hits[:, 0]).all() and len(hits) > 200  # certain hits: none is a miss
    same_queries(a, b, random_rays(p1))


# ------------------------------------------------------------------------------------------------ 2. stale boxes must fail
@pytest.mark.parametrize("name", ["grid", "cow"])
def test_a_mesh_moved_far_away_is_hit_where_it_is_and_missed_where_it_was(gpu, name):
    p0 = mesh(name)
    lo, hi, c, ext = box_of(p0)
    shift = np.array([3.0 * ext, 0.0, 0.0])
    p2 = np.ascontiguousarray(p0 + shift)
    a, b = build(p0, p0), build(p2, p0)
    art.query_rays(a, random_rays(p0))  # A is uploaded, and traversed, where it was
    art.update_triangles(a, p2)
    front = np.array([c[0], c[1], hi[2] + 4.0 * ext])
    step = max(1, len(p0) // NQ)
    now = same_queries(a, b, rays_toward(p2, front + shift, step))
    assert np.isfinite(now[:, 0]).all() and (now[:, 10] >= 2 ** 30).all() and (now[:, 10] < 2 ** 31).all() and len(now) > 200  # every ray hits a triangle
    was = same_queries(a, b, rays_toward(p0, front, step))
    assert np.isinf(was[:, 0]).all() and (was[:, 10] == -1).all() and len(was) > 200
    cam = frame_camera(np.concatenate([p0, p2]))
    assert same_render(render(a, cam), render(b, cam))


# ------------------------------------------------------------------------------------------------ 3. round trip
def test_a_round_trip_of_the_grid_renders_the_untouched_scene(gpu):
    p0 = mesh("grid")
    p1 = twist(p0)
    a, cam = build(p0, p1), frame_camera(p1)
    ref = render(a, cam)
    art.update_triangles(a, p1)
    assert not same_render(render(a, cam), ref)
    art.update_triangles(a, np.ascontiguousarray(p0).reshape(-1, 9))  # the (n, 9) form
    assert same_render(render(a, cam), ref)
    assert same_render(render(build(p0, p1), cam), ref)


@pytest.mark.parametrize("scene", ["cow", "dino", "9"])
def test_builtin_scenes_survive_their_own_vertices_and_a_round_trip(gpu, scene):
    world = art.scene_manager(ASSETS).build(scene)  # scene 9: barycentric textures and per-triangle materials
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    ref = render(world.objects, cam, world.background)
    p0 = art.scene_triangles(world)
    art.update_triangles(world, p0)  # its own vertices: no bit changes
    assert same_render(render(world.objects, cam, world.background), ref)
    assert (bits(art.scene_triangles(world)) == bits(p0)).all()
    art.update_triangles(world, twist(p0))
    moved = render(world.objects, cam, world.background)
    assert not same_render(moved, ref) and kernel_of(moved[2]) == kernel_of(ref[2])
    art.update_triangles(world, p0)
    assert same_render(render(world.objects, cam, world.background), ref)


# ------------------------------------------------------------------------------------------------ 4. device tensors
@pytest.mark.parametrize("name", ["grid", "cow"])
def test_a_device_tensor_on_a_side_stream_then_views_on_that_stream(gpu, name):
    import torch
    p0 = mesh(name)
    p1 = twist(p0)
    a, b = build(p0, p1), build(p1, p1)
    lo, hi, c, ext = box_of(p1)
    cams = [art.camera((c[0] + s * ext, c[1] + 0.8 * ext, c[2] + 2.2 * ext), tuple(c), (0, 1, 0), 40.0, W / H, 0.0, 10.0, 0.0, 1.0) for s in (-1.0, 0.0, 1.0)]
    want, want_sums = art.render_views(b, cams, W, H, SPP, seed=9, background=SKY, accum=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        verts = torch.from_numpy(np.array(p1)).to("cuda", non_blocking=False)
        assert art.update_triangles(a, verts) is None  # enqueued on the side stream
        got = torch.zeros((3, H, W, 3), dtype=torch.uint8, device="cuda")
        sums = torch.zeros((3, H, W, 3), dtype=torch.float64, device="cuda")
        art.render_views(a, cams, W, H, SPP, seed=9, background=SKY, out=got, accum=sums)
    side.synchronize()
    assert (got.cpu().numpy() == want).all() and (bits(sums.cpu().numpy()) == bits(want_sums)).all()
    assert want.max() > 0


def test_a_partial_update_of_the_middle_third(gpu):
    import torch
    p0 = mesh("grid")
    p1 = twist(p0)
    n = len(p0)
    first, last = n // 3, 2 * (n // 3)
    mix = np.array(p0)
    mix[first:last] = p1[first:last]
    a, b, cam = build(p0, p1), build(mix, p1), frame_camera(p1)
    part = torch.from_numpy(np.ascontiguousarray(p1[first:last])).cuda()
    ms = art.update_triangles(a, part, first=first, timing=True)
    assert ms > 0
    assert same_render(render(a, cam), render(b, cam))
    assert (bits(art.scene_triangles(a)) == bits(mix)).all()
    same_queries(a, b, random_rays(p1))


@pytest.mark.parametrize("name", ["grid", "cow"])
def test_a_timed_update_on_a_side_stream_equals_the_host_update(gpu, name):
    # timing on a caller's stream: the call runs there and waits.  Three triangles from the middle of the mesh
    import torch
    p0 = mesh(name)
    p1 = twist(p0)
    first = len(p0) // 2
    part = np.ascontiguousarray(p1[first:first + 3])
    a, b, cam = build(p0, p1), build(p0, p1), frame_camera(p1)
    art.update_triangles(b, part, first=first)  # host buffers
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ms = art.update_triangles(a, torch.from_numpy(part).to("cuda"), first=first, timing=True)
    assert ms > 0
    assert (bits(art.scene_triangles(a)) == bits(art.scene_triangles(b))).all()
    assert (bits(art.scene_triangles(a)[first:first + 3]) == bits(part)).all()
    assert same_render(render(a, cam), render(b, cam))


# ------------------------------------------------------------------------------------------------ 5. loose primitives
def test_loose_triangles_of_an_unmerged_world_are_updated(gpu, options):
    options("compile.world_merge", 0)  # the world stays a list: the floor's two triangles are prim objects (obj_prims)
    p0 = mesh("grid")
    lo, hi, c, ext = box_of(p0)

    def floor(y, tilt):
        q = [(lo[0] - ext, y, lo[2] - ext), (hi[0] + ext, y + tilt, lo[2] - ext), (hi[0] + ext, y + tilt, hi[2] + ext), (lo[0] - ext, y, hi[2] + ext)]
        return np.array([[q[0], q[2], q[1]], [q[0], q[3], q[2]]], np.float64)

    f0, f1 = floor(lo[1] - 0.5, 0.0), floor(lo[1] - 1.5, 1.0)
    a, b = build(p0, p0, f0), build(p0, p0, f1)
    cam = frame_camera(p0)
    before = render(a, cam)
    assert (bits(art.scene_triangles(a)[len(p0):]) == bits(f0)).all()  # the loose triangles follow the mesh's
    art.update_triangles(a, f1, first=len(p0))
    ra, rb = render(a, cam), render(b, cam)
    assert same_render(ra, rb) and not same_render(ra, before)
    down = rays_toward(f1, (c[0], hi[1] + 3.0 * ext, c[2]), 1)
    down = np.concatenate([down, random_rays(np.concatenate([p0, f1]))])
    same_queries(a, b, down)


# ------------------------------------------------------------------------------------------------ 6. the boxes are the specified ones
@pytest.mark.parametrize("name", ["grid", "capsule"])
def test_the_refitted_boxes_are_the_specified_ones(gpu, name):
    a, _, p1, _, _, (nodes0, refs0) = updated_pair(name)
    nodes, refs = art.scene_bvh(a)
    tris = art.scene_triangles(a)
    assert (bits(tris) == bits(p1)).all()
    assert len(nodes) == len(nodes0) and (nodes["child"] == nodes0["child"]).all() and (nodes["pad"] == nodes0["pad"]).all()
    assert (refs == refs0).all()
    changed = sum(int((nodes[f] != nodes0[f]).sum()) for f in ("lox", "hix", "loy", "hiy", "loz", "hiz"))
    assert changed > len(nodes)  # the update did move the boxes
    planes = lambda n, c: (np.array([nodes["lox"][n, c], nodes["loy"][n, c], nodes["loz"][n, c]]),  # noqa: E731
                           np.array([nodes["hix"][n, c], nodes["hiy"][n, c], nodes["hiz"][n, c]]))
    tri_lo, tri_hi = tris.min(1), tris.max(1)
    leaves = inner = 0
    for n in range(len(nodes)):
        for c in range(4):
            code = int(nodes["child"][n, c])
            lo, hi = planes(n, c)
            if code == -1:
                assert (lo == np.finfo(np.float32).max).all() and (hi == -np.finfo(np.float32).max).all()
            elif code < 0:
                first, count = ~code & 0xFFFFFF, (~code >> 24) & 0x7F
                r = refs[first:first + count]
                if not ((r >> 30) == 1).all():
                    continue  # a leaf with a sphere in it: its box is not the triangles' alone
                idx = r & (2 ** 30 - 1)
                wl, wh = conservative_box_np(tri_lo[idx].min(0), tri_hi[idx].max(0))
                assert (lo.view(np.int32) == wl.view(np.int32)).all() and (hi.view(np.int32) == wh.view(np.int32)).all(), (n, c)
                leaves += 1
            else:
                assert code > n
                live = nodes["child"][code] != -1
                wl = np.array([nodes[f][code][live].min() for f in ("lox", "loy", "loz")])
                wh = np.array([nodes[f][code][live].max() for f in ("hix", "hiy", "hiz")])
                assert (lo == wl).all() and (hi == wh).all(), (n, c)
                inner += 1
    assert leaves > len(p1) // 8 and inner == len(nodes) - 1  # every node but the root is some node's child


# ------------------------------------------------------------------------------------------------ 7. save and load
def test_an_updated_scene_is_saved_and_loaded_as_updated(gpu, tmp_path):
    sm = art.scene_manager(ASSETS)
    world = sm.build("cow")
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    ref = render(world.objects, cam, world.background)
    p1 = twist(art.scene_triangles(world))
    art.update_triangles(world, p1)
    moved = render(world.objects, cam, world.background)
    assert not same_render(moved, ref)
    path = tmp_path / "cow_updated.art"
    art.save_scene(world, path)
    loaded = sm.load(path)
    assert (bits(art.scene_triangles(loaded)) == bits(p1)).all()
    assert same_render(render(loaded.objects, cam, world.background), moved)
    # the graph no longer describes the updated scene
    assert lib.rt_scene_dump(world.objects._native, None, 0) == 0 and b"updated" in lib.rt_last_error()
    assert lib.rt_scene_dump(sm.build("cow").objects._native, None, 0) > 0
