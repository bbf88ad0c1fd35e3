"""rt_scene_update_spheres on the GPU.  A scene compiled with spheres S0 and updated to S1 must give, bit for bit, what a
scene compiled fresh with S1 gives -- frames, f64 sums, segment counts, hit records, occlusion bytes -- on every array a
sphere lives in: the LDS scene image (`image`: k_paths, the LDS wavefront kernels, the tile lists), the records and
their leaf-ordered copy (`mixed`: spheres beside a mesh; RT_GLOBAL_SCENE), the prim objects' copies (loose spheres of an
unmerged world, a constant_medium's boundary) and a BVH under translate(rotate_y()) (`xform_media`).  Equality alone
would pass a refit to infinite boxes and, where the spheres only grow, one that keeps stale boxes: rays toward spheres
moved far away (they must hit, and miss where the spheres were), a numpy restatement of every box of the refitted tree and
the image compared byte for byte with the host builder's rule those out.  Frames are 64 x 36 x 8, queries 4096 rays.

Counts used for `image`: a ground sphere of radius 100 and 48 small ones (6 of them moving along y) in one bvh_node: 49
spheres; the ground is hoisted (no node leaf holds its slot), the scene runs k_paths (extend_variant 3, LDS mode 3)
and has tile representatives (rt_tile_candidates > 0 under render.tile_lists = 2)."""
import functools

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import lib
from tests.update_common import (ASSETS, F_LEAF2, F32, H, IMAGE_BYTES, NODE_CAP, NQ, OFF_INVR, OFF_MAT, OFF_MATIDX, OFF_MOV, OFF_REF, OFF_SPH,
                                 REPS_BYTES, SKY, SLOT_CAP, SPP, W, bits, conservative_box_np, covered_slots, engine_for, frame_camera,
                                 grid_triangles, image_spheres, kernel_of, make_sphere, quant, render, same_queries, same_render, v3)

pytestmark = pytest.mark.gpu

XF_ANGLE, XF_OFFSET = 15.0, np.array([-1.0, 0.5, -2.0])


# ------------------------------------------------------------------------------------------------ worlds
# A world is (S0, D, build): S0 (n, 4) its spheres in compiled order, D (n, 3) the motion center1 - center0 of the moving
# ones (0 rows otherwise), build(S) the compiled world with spheres S -- the same call sequence for every S, so that
# material ids agree between A and B.
def sphere_mats():
    return [art.lambertian((0.8, 0.3, 0.3)), art.lambertian(art.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))), art.metal((0.7, 0.6, 0.5), 0.1),
            art.dielectric(1.5), art.diffuse_light((4.0, 4.0, 4.0))]


def image_spec():
    s0, d = image_spheres()

    def build(s):
        art.reset_scene_rng()
        ground, mats = art.lambertian((0.5, 0.5, 0.5)), sphere_mats()
        objs = [make_sphere(s[0], d[0], ground)] + [make_sphere(s[k], d[k], mats[k % 5]) for k in range(1, len(s))]
        w = art.hittable_list()
        w.add(art.bvh_node(objs))
        return art.hittable_list(native=art.compile_world(w, 0))
    return s0, d, build


def mixed_spec():
    rng = np.random.default_rng(22)
    tris = grid_triangles()
    s0, d = np.zeros((22, 4)), np.zeros((22, 3))
    for k in range(20):  # above the height field
        s0[k] = (-2.5 + 1.25 * (k % 5) + rng.uniform(-0.2, 0.2), rng.uniform(2.6, 3.4), -2.0 + 1.3 * (k // 5) + rng.uniform(-0.2, 0.2), rng.uniform(0.2, 0.35))
    s0[20] = (0.0, 9.0, 0.0, 1.5)   # a light above
    s0[21] = (-6.0, 1.5, 0.0, 1.2)  # a mirror beside
    s0 = quant(s0)

    def build(s):
        art.reset_scene_rng()
        tri_mats = [art.lambertian(c) for c in ((0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.3, 0.3, 0.8))]
        mats = sphere_mats()
        light, mirror = art.diffuse_light((4.0, 4.0, 4.0)), art.metal((0.8, 0.8, 0.8), 0.0)
        objs = [art.triangle(t[0], t[1], t[2], tri_mats[i % 3]) for i, t in enumerate(tris)]
        objs += [make_sphere(s[k], d[k], mats[k % 4]) for k in range(20)]
        w = art.hittable_list()
        w.add(art.bvh_node(objs))
        w.add(make_sphere(s[20], d[20], light))
        w.add(make_sphere(s[21], d[21], mirror))
        return art.hittable_list(native=art.compile_world(w, 0))
    return s0, d, build


def xform_media_spec():
    rng = np.random.default_rng(23)
    s0, d = np.zeros((66, 4)), np.zeros((66, 3))
    for k in range(64):
        s0[k] = (-3.5 + (k % 8) + rng.uniform(-0.2, 0.2), rng.uniform(0.3, 1.5), -3.5 + (k // 8) + rng.uniform(-0.2, 0.2), rng.uniform(0.15, 0.3))
    s0[64] = (0.0, 1.0, 4.5, 1.0)   # the medium's boundary
    s0[65] = (5.0, 1.0, 0.0, 0.4)   # a loose sphere moving along x
    d[65, 0] = 0.5
    s0 = quant(s0)

    def build(s):
        art.reset_scene_rng()
        mats = sphere_mats()
        objs = [make_sphere(s[k], d[k], mats[k % 5]) for k in range(64)]
        w = art.hittable_list()
        w.add(art.translate(art.rotate_y(art.bvh_node(objs), XF_ANGLE), v3(XF_OFFSET)))
        w.add(art.constant_medium(make_sphere(s[64], d[64], mats[0]), 0.3, (0.9, 0.9, 0.9)))
        w.add(make_sphere(s[65], d[65], mats[2]))
        return art.hittable_list(native=art.compile_world(w, 0))
    return s0, d, build


SPECS = {"image": image_spec, "mixed": mixed_spec, "xform_media": xform_media_spec}


@functools.lru_cache(maxsize=None)
def spec(name):
    s0, d, build = SPECS[name]()
    s0.setflags(write=False)
    d.setflags(write=False)
    return s0, d, build


def jitter(s0, seed=31):
    """S1: the centres moved by up to 2 radii per axis and the radii scaled by [0.6, 1.5], seeded.  A sphere of radius > 10
    (the ground) moves by up to 1 and keeps its top where it was, so that the frame still shows the scene."""
    rng = np.random.default_rng(seed)
    s = np.array(s0)
    big = s0[:, 3] > 10.0
    s[:, :3] += rng.uniform(-2.0, 2.0, (len(s), 3)) * np.where(big, 0.5, s0[:, 3])[:, None]
    s[:, 3] *= rng.uniform(0.6, 1.5, len(s))
    s[big, 1] = s0[big, 1] + s0[big, 3] - s[big, 3]
    return quant(s)


def world_centres(name, s, d, tm=0.5):
    """The centres at ray time tm in world space (xform_media's first 64 spheres sit under translate(rotate_y()))."""
    c = s[:, :3] + tm * d
    if name == "xform_media":
        a = np.radians(XF_ANGLE)
        x, z = c[:64, 0].copy(), c[:64, 2].copy()
        c[:64, 0], c[:64, 2] = np.cos(a) * x + np.sin(a) * z, -np.sin(a) * x + np.cos(a) * z
        c[:64] += XF_OFFSET
    return c


def solid(name, n):
    """The spheres a ray toward their centre certainly hits: all but a medium's boundary."""
    keep = np.ones(n, bool)
    if name == "xform_media":
        keep[64] = False
    return keep


def rays_to(points, origin, tm=0.5):
    origin = np.broadcast_to(np.asarray(origin, np.float64), points.shape)
    rays = np.zeros((len(points), 7))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = origin, points - origin, tm
    return rays


def random_rays(lo, hi, seed=11):
    c, ext = 0.5 * (lo + hi), float((hi - lo).max())
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(NQ, 3))
    o = c + 3.0 * ext * o / np.linalg.norm(o, axis=1, keepdims=True)
    target = rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, (NQ, 3))
    rays = np.zeros((NQ, 7))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, target - o, rng.uniform(0, 1, NQ)
    return rays


def small_box(s):
    small = s[:, 3] < 10.0
    return (s[small, :3] - s[small, 3:4]).min(0), (s[small, :3] + s[small, 3:4]).max(0)


@functools.lru_cache(maxsize=None)
def updated_pair(name):
    """Case 1's worlds: A = build(S0) rendered, then updated to S1 from a host array; B = build(S1).  Shared by the tests
    that only read them."""
    s0, d, build = spec(name)
    s1 = jitter(s0)
    s1.setflags(write=False)
    a = build(s0)
    assert (bits(art.scene_spheres(a)) == bits(s0)).all()  # the compiled order is the order the spec lists them in
    cam = frame_camera(name)
    before = render(a, cam)
    bvh_before = art.scene_bvh(a)
    image_before = art.scene_lds_image(a)
    art.update_spheres(a, s1)
    b = build(s1)
    return a, b, s1, cam, before, bvh_before, image_before


# ------------------------------------------------------------------------------------------------ 1. equality with a fresh compile
def check_pair(name, a, b, s1, d, cam, before):
    ra, rb = render(a, cam), render(b, cam)
    assert kernel_of(ra[2]) == kernel_of(before[2])  # A runs what it ran
    assert same_render(ra, rb), (int((ra[0] != rb[0]).sum()), ra[2]["segments"], rb[2]["segments"])
    assert not same_render(ra, before) and ra[0].max() > 0  # the update is visible
    assert (bits(art.scene_spheres(a)) == bits(s1)).all()
    keep = solid(name, len(s1))
    lo, hi = small_box(s1)
    cam_rays, _ = art.camera_rays(cam, W, H, 2)
    for g in (False, True):  # with and without RT_GLOBAL_SCENE
        same_queries(a, b, np.ascontiguousarray(cam_rays[:NQ]), global_scene=g)
        hits = same_queries(a, b, rays_to(world_centres(name, s1, d)[keep], (0.5, 7.0, 40.0)), global_scene=g)
        assert np.isfinite(hits[:, 0]).all() and len(hits) == keep.sum()  # certain hits: none is a miss
        same_queries(a, b, random_rays(lo, hi), global_scene=g)
    return ra


@pytest.mark.parametrize("name", ["image", "mixed", "xform_media"])
def test_an_updated_scene_equals_the_fresh_compile_of_its_spheres(gpu, name):
    a, b, s1, cam, before, _, image_before = updated_pair(name)
    ra = check_pair(name, a, b, s1, spec(name)[1], cam, before)
    if name == "image":
        assert ra[2]["extend_variant"] == 3 and ra[2]["kernel_lds_mode"] == 3 and image_before is not None
        nodes, refs = art.scene_bvh(a)
        loose = ~covered_slots(nodes, len(refs))
        assert loose.sum() >= 1 and 0 in (refs[loose] & (2 ** 30 - 1))  # the ground is hoisted: no node leaf holds its slot
    elif name == "mixed":
        assert ra[2]["extend_variant"] == 4 and image_before is None
    views_a = art.render_views(a, [cam, frame_camera("mixed")], W, H, SPP, seed=9, background=SKY, accum=True)
    views_b = art.render_views(b, [cam, frame_camera("mixed")], W, H, SPP, seed=9, background=SKY, accum=True)
    assert (views_a[0] == views_b[0]).all() and (bits(views_a[1]) == bits(views_b[1])).all()
    rays = random_rays(*small_box(s1), seed=12)[:1024]
    for g in (False, True):
        rad_a, rad_b = art.radiance_rays(a, rays, spp=2, seed=3, background=SKY, global_scene=g), art.radiance_rays(b, rays, spp=2, seed=3, background=SKY, global_scene=g)
        assert (bits(rad_a) == bits(rad_b)).all()
    ga, gb = engine_for(a, cam).render_guides(), engine_for(b, cam).render_guides()
    assert (bits(ga) == bits(gb)).all()


@pytest.mark.parametrize("form", [{"wavefront": True}, {"split_shade": True}, {"global_scene": True}, {"wavefront": True, "global_scene": True}])
def test_every_engine_form_of_the_image_scene_sees_the_update(gpu, form):
    a, b, s1, cam, before, _, _ = updated_pair("image")
    ra, rb = render(a, cam, **form), render(b, cam, **form)
    assert same_render(ra, rb), (form, int((ra[0] != rb[0]).sum()))
    assert same_render(ra, render(a, cam)) and not same_render(ra, before)  # every form computes the same frame


def test_tile_lists_and_noise_target_of_the_image_scene_follow_the_update(gpu, options):
    a, b, s1, cam, before, _, _ = updated_pair("image")
    options("render.tile_lists", 2)
    ea, eb = engine_for(a, cam), engine_for(b, cam)
    ta, tb = ea.tile_candidates(), eb.tile_candidates()
    assert ta is not None and tb is not None and (ta == tb).all() and ta.sum() > 0 and (ta > 0).any()
    ra, rb = render(a, cam), render(b, cam)
    assert same_render(ra, rb) and ra[2]["extend_variant"] == 3
    options("render.tile_lists", 0)
    assert same_render(render(a, cam), ra)  # the lists change no bit
    outs = []
    for eng in (ea, eb):
        img, acc, cnt = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.float64), np.zeros((H, W), np.int32)
        eng.run_noise_target(img, accum=acc, counts=cnt, min_spp=4, step_spp=4)
        outs.append((img, acc, cnt))
    assert (outs[0][0] == outs[1][0]).all() and (bits(outs[0][1]) == bits(outs[1][1])).all() and (outs[0][2] == outs[1][2]).all()


def test_loose_spheres_of_an_unmerged_world_are_updated(gpu, options):
    options("compile.world_merge", 0)  # the world stays a list: the two loose spheres are prim objects (obj_prims)
    s0, d, build = spec("mixed")
    s1 = jitter(s0)
    a, cam = build(s0), frame_camera("mixed")
    before = render(a, cam)
    art.update_spheres(a, s1)
    b = build(s1)
    check_pair("mixed", a, b, s1, d, cam, before)
    # the loose spheres alone, back where they were: a partial update through obj_prims
    art.update_spheres(a, np.ascontiguousarray(s0[20:]), first=20)
    mix = np.array(s1)
    mix[20:] = s0[20:]
    assert same_render(render(a, cam), render(build(mix), cam))


# ------------------------------------------------------------------------------------------------ 2. stale boxes must fail
@pytest.mark.parametrize("name,global_scene", [("image", False), ("image", True), ("mixed", False)])
def test_spheres_moved_far_away_are_hit_where_they_are_and_missed_where_they_were(gpu, name, global_scene):
    s0, d, build = spec(name)
    ext = float(((s0[:, :3] + s0[:, 3:4]).max(0) - (s0[:, :3] - s0[:, 3:4]).min(0)).max())
    shift = np.array([3.0 * ext, 0.0, 0.0])
    s2 = np.array(s0)
    s2[:, :3] += shift
    a, b = build(s0), build(s2)
    lo, hi = small_box(s0)
    art.query_rays(a, random_rays(lo, hi), global_scene=global_scene)  # A is uploaded, and traversed, where it was
    art.update_spheres(a, s2)
    # one horizontal ray per small sphere, at its centre's height at the ray's time: above the ground's top and the mesh
    small = s0[:, 3] < 10.0
    was_at = world_centres(name, s0, d)[small]
    front = was_at + np.array([0.0, 0.0, 4.0 * ext])
    now = same_queries(a, b, rays_to(was_at + shift, front + shift), global_scene=global_scene)
    assert np.isfinite(now[:, 0]).all() and (now[:, 10] >= 0).all() and (now[:, 10] < 2 ** 30).all() and len(now) == small.sum()  # every ray hits a sphere
    was = same_queries(a, b, rays_to(was_at, front), global_scene=global_scene)
    assert np.isinf(was[:, 0]).all() and (was[:, 10] == -1).all()
    cam = frame_camera(name)
    assert same_render(render(a, cam, global_scene=global_scene), render(b, cam, global_scene=global_scene))


# ------------------------------------------------------------------------------------------------ 3. the image, byte for byte
def planes_that_stay(img):
    child = img[9 * NODE_CAP * 16:10 * NODE_CAP * 16]
    return [child, img[OFF_MOV:OFF_REF], img[OFF_REF:OFF_MATIDX], img[OFF_MATIDX:OFF_MAT], img[OFF_MAT:OFF_INVR], img[IMAGE_BYTES:]]


def test_the_image_is_the_host_builders_byte_for_byte(gpu):
    s0, d, build = spec("image")
    a = build(s0)
    img0 = art.scene_lds_image(a)
    assert img0 is not None and img0.dtype == np.uint8 and len(img0) == IMAGE_BYTES + REPS_BYTES == 117264
    assert (img0 == art.scene_lds_image(a, rebuilt=True)).all()
    assert int(img0[IMAGE_BYTES:IMAGE_BYTES + 4].view(np.uint32)[0]) == len(s0)  # one tile representative per sphere
    s1 = jitter(s0)
    art.update_spheres(a, s1)
    img1, re1 = art.scene_lds_image(a), art.scene_lds_image(a, rebuilt=True)
    assert (img1 == re1).all(), np.flatnonzero(img1 != re1)[:8]
    assert (img1[:9 * NODE_CAP * 16] != img0[:9 * NODE_CAP * 16]).any() and (img1[OFF_SPH:OFF_MOV] != img0[OFF_SPH:OFF_MOV]).any()
    assert (img1[OFF_INVR:IMAGE_BYTES] != img0[OFF_INVR:IMAGE_BYTES]).any()
    for p0, p1 in zip(planes_that_stay(img0), planes_that_stay(img1)):
        assert (p0 == p1).all()
    # what a fresh compile of S1 holds per sphere, whatever slots its own tree gives them: compare through the slot's index field
    fresh = build(s1)
    for img, n_slots in ((img1, len(art.scene_bvh(a)[1])), (art.scene_lds_image(fresh), len(art.scene_bvh(fresh)[1]))):
        idx = img[OFF_REF:OFF_MATIDX].view(np.uint32) & (2 ** 19 - 1)
        assert n_slots >= len(s0)
        xy = img[OFF_SPH:OFF_SPH + SLOT_CAP * 16].view(np.float64).reshape(-1, 2)[:n_slots]
        zr = img[OFF_SPH + SLOT_CAP * 16:OFF_MOV].view(np.float64).reshape(-1, 2)[:n_slots]
        inv = img[OFF_INVR:IMAGE_BYTES].view(np.float64)[:n_slots]
        k = idx[:n_slots]
        assert (bits(xy[:, 0]) == bits(s1[k, 0] + d[k, 0])).all() and (bits(xy[:, 1]) == bits(s1[k, 1])).all()
        assert (bits(zr[:, 0]) == bits(s1[k, 2] + d[k, 2])).all() and (bits(zr[:, 1]) == bits(s1[k, 3] * s1[k, 3])).all()
        assert (bits(inv) == bits(1.0 / s1[k, 3])).all()
    # a second, partial update: the middle third
    n = len(s0)
    first, last = n // 3, 2 * (n // 3)
    s2 = jitter(s0, seed=77)
    art.update_spheres(a, np.ascontiguousarray(s2[first:last]), first=first)
    img2, re2 = art.scene_lds_image(a), art.scene_lds_image(a, rebuilt=True)
    assert (img2 == re2).all(), np.flatnonzero(img2 != re2)[:8]
    assert (img2 != img1).any()
    for p0, p2 in zip(planes_that_stay(img0), planes_that_stay(img2)):
        assert (p0 == p2).all()
    mix = np.array(s1)
    mix[first:last] = s2[first:last]
    assert (bits(art.scene_spheres(a)) == bits(mix)).all()
    cam = frame_camera("image")
    assert same_render(render(a, cam), render(build(mix), cam))


# ------------------------------------------------------------------------------------------------ 4. the boxes are the specified ones
def sphere_boxes_np(s, d):
    """refit.h sphere_box: c -+ r, or for a moving sphere (unit shutter here) the union of the boxes at t = 0 and t = 1."""
    c, r = s[:, :3], s[:, 3:4]
    moving = d.any(1)[:, None]
    c0, c1 = c + 0.0 * d, c + 1.0 * d
    return np.where(moving, np.minimum(c0 - r, c1 - r), c - r), np.where(moving, np.maximum(c0 + r, c1 + r), c + r)


@pytest.mark.parametrize("name", ["image", "xform_media"])
def test_the_refitted_boxes_are_the_specified_ones(gpu, name):
    a, _, s1, _, _, (nodes0, refs0), _ = updated_pair(name)
    d = spec(name)[1]
    nodes, refs = art.scene_bvh(a)
    assert len(nodes) == len(nodes0) and (nodes["child"] == nodes0["child"]).all() and (nodes["pad"] == nodes0["pad"]).all()
    assert (refs == refs0).all() and ((refs >> 30) == 0).all()
    changed = sum(int((nodes[f] != nodes0[f]).sum()) for f in ("lox", "hix", "loy", "hiy", "loz", "hiz"))
    assert changed > len(nodes)  # the update did move the boxes
    planes = lambda n, c: (np.array([nodes["lox"][n, c], nodes["loy"][n, c], nodes["loz"][n, c]]),  # noqa: E731
                           np.array([nodes["hix"][n, c], nodes["hiy"][n, c], nodes["hiz"][n, c]]))
    sph_lo, sph_hi = sphere_boxes_np(s1, d)
    leaves = inner = 0
    for n in range(len(nodes)):
        for c in range(4):
            code = int(nodes["child"][n, c])
            lo, hi = planes(n, c)
            if code == -1:
                assert (lo == np.finfo(F32).max).all() and (hi == -np.finfo(F32).max).all()
            elif code < 0:
                first, count = ~code & 0xFFFFFF, (~code >> 24) & 0x7F
                idx = refs[first:first + count] & (2 ** 30 - 1)
                wl, wh = conservative_box_np(sph_lo[idx].min(0), sph_hi[idx].max(0))
                assert (lo.view(np.int32) == wl.view(np.int32)).all() and (hi.view(np.int32) == wh.view(np.int32)).all(), (n, c)
                leaves += 1
            else:
                assert code > n
                live = nodes["child"][code] != -1
                wl = np.array([nodes[f][code][live].min() for f in ("lox", "loy", "loz")])
                wh = np.array([nodes[f][code][live].max() for f in ("hix", "hiy", "hiz")])
                assert (lo == wl).all() and (hi == wh).all(), (n, c)
                inner += 1
    assert leaves >= 12 and inner == len(nodes) - 1  # every node but the root is some node's child


# ------------------------------------------------------------------------------------------------ 5. round trips
def test_a_round_trip_renders_the_untouched_scene(gpu):
    for name in ("image", "xform_media"):
        s0, d, build = spec(name)
        a, cam = build(s0), frame_camera(name)
        ref = render(a, cam)
        art.update_spheres(a, jitter(s0))
        assert not same_render(render(a, cam), ref)
        art.update_spheres(a, np.array(s0))
        assert same_render(render(a, cam), ref)
        assert (bits(art.scene_spheres(a)) == bits(s0)).all()
        if name == "image":  # the sphere planes are the fresh build's again (the box planes are a refit's: as tight, not the same bits)
            back, fresh = art.scene_lds_image(a), art.scene_lds_image(build(s0))
            assert (back[OFF_SPH:] == fresh[OFF_SPH:]).all() and (back == art.scene_lds_image(a, rebuilt=True)).all()


@pytest.mark.parametrize("scene", ["1", "c1", "final"])
def test_builtin_scenes_survive_their_own_spheres_and_a_round_trip(gpu, scene):
    # scene 1: the image, 874 slots, moving spheres, the hoisted ground; final: 1008 spheres under transforms, a
    # sphere-bounded medium, an x-moving sphere
    sm = art.scene_manager(ASSETS)
    world, untouched = sm.build(scene), sm.build(scene)
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    ref = render(untouched.objects, cam, world.background)
    s0 = art.scene_spheres(world)
    assert len(s0) == world.info["spheres"] > 0
    image0 = art.scene_lds_image(world)
    art.update_spheres(world, s0)  # its own spheres: no bit changes
    same = render(world.objects, cam, world.background)
    assert same_render(same, ref) and kernel_of(same[2]) == kernel_of(ref[2])
    assert (bits(art.scene_spheres(world)) == bits(s0)).all()
    if scene in ("1", "c1"):
        image = art.scene_lds_image(world)
        assert image0 is not None and (image[OFF_SPH:] == image0[OFF_SPH:]).all() and same[2]["extend_variant"] == 3
        assert (image[9 * NODE_CAP * 16:OFF_SPH] == image0[9 * NODE_CAP * 16:OFF_SPH]).all()  # the child codes
        assert (art.scene_lds_image(world, rebuilt=True) == image).all()
    else:
        assert image0 is None
    moved = np.array(s0)
    moved[:, 1] += 0.25 * moved[:, 3]
    art.update_spheres(world, moved)
    up = render(world.objects, cam, world.background)
    assert not same_render(up, ref) and kernel_of(up[2]) == kernel_of(ref[2])
    art.update_spheres(world, s0)
    assert same_render(render(world.objects, cam, world.background), ref)


# ------------------------------------------------------------------------------------------------ 6. streams and partial updates
@pytest.mark.parametrize("name", ["image", "mixed"])
def test_a_device_tensor_on_a_side_stream_then_views_on_that_stream(gpu, name):
    import torch
    s0, d, build = spec(name)
    s1 = jitter(s0)
    a, b = build(s0), build(s1)
    cams = [frame_camera(name), frame_camera("mixed"), frame_camera("xform_media")]
    want, want_sums = art.render_views(b, cams, W, H, SPP, seed=9, background=SKY, accum=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        vals = torch.from_numpy(np.array(s1)).to("cuda", non_blocking=False)
        assert art.update_spheres(a, vals) is None  # enqueued on the side stream
        got = torch.zeros((3, H, W, 3), dtype=torch.uint8, device="cuda")
        sums = torch.zeros((3, H, W, 3), dtype=torch.float64, device="cuda")
        art.render_views(a, cams, W, H, SPP, seed=9, background=SKY, out=got, accum=sums)
    side.synchronize()
    assert (got.cpu().numpy() == want).all() and (bits(sums.cpu().numpy()) == bits(want_sums)).all()
    assert want.max() > 0


@pytest.mark.parametrize("name", ["image", "xform_media"])
def test_a_partial_update_of_the_middle_third(gpu, name):
    import torch
    s0, d, build = spec(name)
    s1 = jitter(s0)
    n = len(s0)
    first, last = n // 3, 2 * (n // 3)
    mix = np.array(s0)
    mix[first:last] = s1[first:last]
    a, b, cam = build(s0), build(mix), frame_camera(name)
    part = torch.from_numpy(np.ascontiguousarray(s1[first:last])).cuda()
    ms = art.update_spheres(a, part, first=first, timing=True)
    assert ms > 0
    assert same_render(render(a, cam), render(b, cam))
    assert (bits(art.scene_spheres(a)) == bits(mix)).all()  # the rest stays in place
    same_queries(a, b, random_rays(*small_box(mix)))


@pytest.mark.parametrize("name", ["image", "mixed"])
def test_a_timed_update_on_a_side_stream_equals_the_host_update(gpu, name):
    # timing on a caller's stream: the call runs there and waits.  Three spheres from the middle of the scene
    import torch
    s0, d, build = spec(name)
    s1 = jitter(s0)
    first = len(s0) // 2
    part = np.ascontiguousarray(s1[first:first + 3])
    a, b, cam = build(s0), build(s0), frame_camera(name)
    art.update_spheres(b, part, first=first)  # host buffers
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ms = art.update_spheres(a, torch.from_numpy(part).to("cuda"), first=first, timing=True)
    assert ms > 0
    assert (bits(art.scene_spheres(a)) == bits(art.scene_spheres(b))).all()
    assert (bits(art.scene_spheres(a)[first:first + 3]) == bits(part)).all()
    assert same_render(render(a, cam), render(b, cam))
    if name == "image":
        assert (art.scene_lds_image(a) == art.scene_lds_image(b)).all()


# ------------------------------------------------------------------------------------------------ 7. pad slots
def test_pad_slots_of_a_pair_aligned_scene_stay_out_of_a_sphere_update(gpu):
    """The capsule's 10 200 triangles (more than 8192 references: the scene runs an F_LEAF2 kernel on a padded copy of the
    references, whose pad slots hold reference 0 = sphere 0) with three spheres in the same bvh_node."""
    tris = art.scene_triangles(art.scene_manager(ASSETS).build("9"))
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    c, ext = 0.5 * (lo + hi), float((hi - lo).max())
    s0 = quant(np.array([[c[0], hi[1] + 2.0 * ext, c[2], 0.5 * ext], [lo[0] - ext, c[1], c[2], 0.4 * ext], [hi[0] + 0.8 * ext, c[1], c[2], 0.3 * ext]]))
    s1 = jitter(s0, seed=5)
    s1[:, :3] = quant(s0[:, :3] + (s1[:, :3] - s0[:, :3]) * 0.2)  # stay clear of the mesh

    def build(s):
        art.reset_scene_rng()
        mats = [art.lambertian(col) for col in ((0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.3, 0.3, 0.8))]
        sm = [art.diffuse_light((4.0, 4.0, 4.0)), art.metal((0.8, 0.8, 0.8), 0.0), art.dielectric(1.5)]
        objs = [art.sphere(v3(s[k, :3]), float(s[k, 3]), sm[k]) for k in range(3)]
        objs += [art.triangle(t[0], t[1], t[2], mats[i % 3]) for i, t in enumerate(tris)]
        w = art.hittable_list()
        w.add(art.bvh_node(objs))
        return art.hittable_list(native=art.compile_world(w, 0))

    a = build(s0)
    cam = art.camera((c[0] + 0.4 * ext, c[1] + 0.9 * ext, c[2] + 3.5 * ext), tuple(c), (0, 1, 0), 40.0, W / H, 0.0, 10.0, 0.0, 1.0)
    before = render(a, cam)
    assert before[2]["kernel_features"] & F_LEAF2
    nodes0, refs0 = art.scene_bvh(a)
    pads = ~covered_slots(nodes0, len(refs0))
    assert pads.sum() > 100 and (refs0[pads] == 0).sum() > 100  # pad slots exist, and read as sphere 0
    art.update_spheres(a, s1)
    b = build(s1)
    ra, rb = render(a, cam), render(b, cam)
    assert same_render(ra, rb) and not same_render(ra, before) and kernel_of(ra[2]) == kernel_of(before[2])
    nodes1, refs1 = art.scene_bvh(a)
    assert (refs1 == refs0).all() and (nodes1["child"] == nodes0["child"]).all() and (nodes1["pad"] == nodes0["pad"]).all()
    assert (bits(art.scene_spheres(a)) == bits(s1)).all()
    hits = same_queries(a, b, rays_to(np.concatenate([s1[:, :3], tris.mean(1)[::40]]), (c[0], c[1] + 0.5 * ext, c[2] + 6.0 * ext)))
    assert np.isfinite(hits[:3, 0]).all()  # toward the three spheres' centres: certain hits
    same_queries(a, b, random_rays(lo - ext, hi + ext))


# ------------------------------------------------------------------------------------------------ 8. save and load
def test_an_updated_scene_is_saved_and_loaded_as_updated(gpu, tmp_path):
    sm = art.scene_manager(ASSETS)
    s0, d, build = spec("image")
    s1 = jitter(s0)
    a, cam = build(s0), frame_camera("image")
    ref = render(a, cam)
    art.update_spheres(a, s1)
    moved = render(a, cam)
    assert not same_render(moved, ref)
    path = tmp_path / "image_updated.art"
    art.save_scene(a, path)
    loaded = sm.load(path)
    assert (bits(art.scene_spheres(loaded)) == bits(s1)).all()
    got = render(loaded.objects, cam)
    assert same_render(got, moved) and kernel_of(got[2]) == kernel_of(moved[2])
    assert (art.scene_lds_image(loaded) == art.scene_lds_image(a)).all()
    # the graph no longer describes the updated scene
    assert lib.rt_scene_dump(a._native, None, 0) == 0 and b"updated" in lib.rt_last_error()
    assert lib.rt_scene_dump(build(s0)._native, None, 0) > 0
