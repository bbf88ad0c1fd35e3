"""rt_scene_update_materials / rt_scene_update_textures on the GPU.  A scene compiled with values V0 and updated to V1
must give, bit for bit, what a scene compiled fresh from the same call sequence with V1 gives -- frames, f64 sums, segment
counts, views, radiance, guides, hit records -- through every copy a value has on the device: the records, the solid
colour inlined into a MATF_SOLID record (`mixed`, and RT_GLOBAL_SCENE on `image`) and the LDS scene image's shading table
(`image`: k_paths, the LDS wavefront kernels, the tile lists).  Frames are 64 x 36 x 8, queries 4096 rays, seed 5.

A world is build(M, T[, S]): M (n, 5) and T (n, 4) in scene_materials' / scene_textures' layout, read by running id as the
constructors are called (None: the literals at the call sites, which are V0), so the ids, and the perlin tables drawn
after art.reset_scene_rng(), agree between A and B.  Every build asserts that each object's .id is the running index.

V1 (v1()): every solid colour and metal albedo redrawn, seeded, in [0.05, 0.95]^3 (a colour only lights use in [1, 8]^3),
fuzz in [0, 0.6] and the last metal's 1.5 (which must behave as 1), ir in [1.2, 2.4] and the last dielectric's 0.75, noise
scale 4 -> 1.5.  Fields a record's type ignores keep V0's values."""
import functools

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd._lib import lib
from tests.update_common import (ASSETS, H, NQ, OFF_INVR, OFF_MAT, SKY, SPP, W, bits, engine_for, frame_camera, grid_triangles, image_spheres,
                                 kernel_of, make_sphere, quant, render, same_render, v3)

pytestmark = pytest.mark.gpu

LAMBERTIAN, METAL, DIELECTRIC, LIGHT, ISOTROPIC = range(5)
SOLID, CHECKER, NOISE, IMAGE, BARY = range(5)


# ------------------------------------------------------------------------------------------------ worlds
class Maker:
    """The material and texture constructors with their values taken from M / T by running id."""

    def __init__(self, M, T):
        self.M, self.T, self.nm, self.nt = M, T, 0, 0

    def _tex(self, t):
        assert t.id == self.nt  # a compiled texture index is the graph's id
        self.nt += 1
        return t

    def _mat(self, m):
        assert m.id == self.nm
        self.nm += 1
        return m

    def solid(self, c):
        return self._tex(art.solid_color(*v3(c if self.T is None else self.T[self.nt, :3])))

    def checker(self, even, odd):
        return self._tex(art.checker_texture(even, odd))

    def noise(self, scale):
        return self._tex(art.noise_texture(float(scale if self.T is None else self.T[self.nt, 3])))

    def image(self, texels):
        return self._tex(art.image_texture(texels))

    def lambertian(self, tex):
        return self._mat(art.lambertian(tex))

    def light(self, tex):
        return self._mat(art.diffuse_light(tex))

    def metal(self, albedo, fuzz):
        if self.M is not None:
            albedo, fuzz = self.M[self.nm, :3], self.M[self.nm, 3]
        return self._mat(art.metal(v3(albedo), float(fuzz)))

    def dielectric(self, ir):
        return self._mat(art.dielectric(float(ir if self.M is None else self.M[self.nm, 4])))

    def medium(self, boundary, density, tex):
        self.nm += 1  # the medium's isotropic material is an ordinary entry, made here
        return art.constant_medium(boundary, density, tex)


def sphere_mats(mk):
    """Eight materials over four textures; `shared` colours a lambertian, a diffuse_light and the checker's even child."""
    shared = mk.solid((0.8, 0.3, 0.3))
    return [mk.lambertian(shared), mk.lambertian(mk.checker(shared, mk.solid((0.9, 0.9, 0.9)))), mk.metal((0.7, 0.6, 0.5), 0.1), mk.dielectric(1.5),
            mk.light(mk.solid((4.0, 4.0, 4.0))), mk.light(shared), mk.metal((0.8, 0.8, 0.8), 0.0), mk.dielectric(1.5)], shared


IMAGE_S0, IMAGE_D = image_spheres()


def build_image(M=None, T=None, S=None):
    s = IMAGE_S0 if S is None else S
    art.reset_scene_rng()
    mk = Maker(M, T)
    ground = mk.lambertian(mk.solid((0.5, 0.5, 0.5)))
    mats, shared = sphere_mats(mk)
    objs = [make_sphere(s[0], IMAGE_D[0], ground)] + [make_sphere(s[k], IMAGE_D[k], mats[k % 8]) for k in range(1, len(s))]
    w = art.hittable_list()
    w.add(art.bvh_node(objs))
    world = art.hittable_list(native=art.compile_world(w, 0))
    world.shared_id, world.counts = shared.id, (mk.nm, mk.nt)
    return world


def mixed_spheres():
    rng = np.random.default_rng(22)
    s = np.zeros((20, 4))
    for k in range(20):  # above the height field
        s[k] = (-2.5 + 1.25 * (k % 5) + rng.uniform(-0.2, 0.2), rng.uniform(2.6, 3.4), -2.0 + 1.3 * (k // 5) + rng.uniform(-0.2, 0.2), rng.uniform(0.2, 0.35))
    return quant(s)


TRIS, MIXED_S = grid_triangles(), mixed_spheres()
TEXELS = (np.arange(8 * 8 * 3, dtype=np.uint32).reshape(8, 8, 3) * 37 % 251).astype(np.uint8)  # 8 x 8 synthetic texels: no update touches them


def build_mixed(M=None, T=None, S=None):
    assert S is None
    art.reset_scene_rng()
    mk = Maker(M, T)
    tri_mats = [mk.lambertian(mk.solid(c)) for c in ((0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.3, 0.3, 0.8))]
    mats, shared = sphere_mats(mk)
    mats.append(mk.lambertian(mk.noise(4.0)))
    picture = mk.lambertian(mk.image(TEXELS))
    crate = mk.lambertian(mk.solid((0.7, 0.5, 0.2)))
    objs = [art.triangle(t[0], t[1], t[2], tri_mats[i % 3]) for i, t in enumerate(TRIS)]
    objs += [art.sphere(v3(MIXED_S[k, :3]), float(MIXED_S[k, 3]), mats[k % 9]) for k in range(20)]
    w = art.hittable_list()
    w.add(art.bvh_node(objs))
    w.add(art.xz_rect(-5.0, -3.2, -2.0, 2.0, 0.2, picture))
    w.add(art.box((3.3, 0.0, -1.0), (4.6, 1.6, 0.6), crate))
    w.add(mk.medium(art.sphere((-4.0, 2.8, 1.0), 1.0, crate), 0.6, mk.solid((0.9, 0.9, 0.9))))
    w.add(art.sphere((0.0, 9.0, 0.0), 1.5, mk.light(mk.solid((4.0, 4.0, 4.0)))))
    world = art.hittable_list(native=art.compile_world(w, 0))
    world.shared_id, world.counts = shared.id, (mk.nm, mk.nt)
    return world


BUILD = {"image": build_image, "mixed": build_mixed}


def v1(M0, Md, T0, Td, seed=41):
    """V1 from V0 and the descriptions (module docstring); fields a record ignores keep V0's values."""
    rng = np.random.default_rng(seed)
    M, T = np.array(M0), np.array(T0)
    lit = {int(t) for ty, t in Md if ty == LIGHT}
    unlit = {int(t) for ty, t in Md if ty in (LAMBERTIAN, ISOTROPIC)} | {int(c) for ty, e, o in Td if ty == CHECKER for c in (e, o)}
    for k, (ty, _, _) in enumerate(Td):
        if ty == SOLID:
            T[k, :3] = rng.uniform(1.0, 8.0, 3) if k in lit - unlit else rng.uniform(0.05, 0.95, 3)
        elif ty == NOISE:
            assert T0[k, 3] == 4.0
            T[k, 3] = 1.5
    for k, (ty, _) in enumerate(Md):
        if ty == METAL:
            M[k, :3], M[k, 3] = rng.uniform(0.05, 0.95, 3), rng.uniform(0.0, 0.6)
        elif ty == DIELECTRIC:
            M[k, 4] = rng.uniform(1.2, 2.4)
    M[np.flatnonzero(Md[:, 0] == METAL)[-1], 3] = 1.5
    M[np.flatnonzero(Md[:, 0] == DIELECTRIC)[-1], 4] = 0.75
    return M, T


def held(M):
    """What the scene holds after taking M: fuzz clamped as SceneGraph::metal clamps it."""
    out = np.array(M)
    out[:, 3] = np.where(out[:, 3] < 1.0, out[:, 3], 1.0)
    return out


@functools.lru_cache(maxsize=None)
def values(name):
    """(M0, Md, T0, Td, M1, T1) of a world, read-only."""
    a = BUILD[name]()
    (M0, Md), (T0, Td) = art.scene_materials(a), art.scene_textures(a)
    assert (len(M0), len(T0)) == a.counts  # every constructor call made one entry, the medium's isotropic included
    M1, T1 = v1(M0, Md, T0, Td)
    out = (M0, Md, T0, Td, M1, T1)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def updated_pair(name):
    """Case 1's worlds: A = build(V0) rendered, then updated to V1 from host arrays; B = build(V1).  Shared by the tests
    that only read them."""
    M0, Md, T0, Td, M1, T1 = values(name)
    a = BUILD[name](M0, T0)  # V0 through the arrays: the same scene as the literals give
    cam = frame_camera(name)
    before = render(a, cam)
    assert same_render(before, render(BUILD[name](), cam))
    image_before = art.scene_lds_image(a)
    art.update_materials(a, M1)
    art.update_textures(a, T1)
    b = BUILD[name](M1, T1)
    return a, b, cam, before, image_before


def same_queries(a, b, rays, **kw):
    ra, rb = art.query_rays(a, rays, **kw).records, art.query_rays(b, rays, **kw).records
    assert ra.shape == (len(rays), 12)
    assert (bits(ra) == bits(rb)).all(), int((bits(ra) != bits(rb)).any(1).sum())
    return ra


def check_pair(a, b, cam, name):
    """Every call of the contract but the engine forms: A's bits are B's."""
    ra, rb = render(a, cam), render(b, cam)
    assert same_render(ra, rb), (int((ra[0] != rb[0]).sum()), ra[2]["segments"], rb[2]["segments"])
    assert kernel_of(ra[2]) == kernel_of(rb[2])
    cams = [cam, frame_camera("mixed" if name == "image" else "image"), frame_camera("side")]
    cam_rays, _ = art.camera_rays(cam, W, H, 2)
    rays = np.ascontiguousarray(cam_rays[:NQ])
    for g in (False, True):  # with and without RT_GLOBAL_SCENE
        rad_a = art.radiance_rays(a, rays[:1024], spp=2, seed=3, background=SKY, global_scene=g)
        rad_b = art.radiance_rays(b, rays[:1024], spp=2, seed=3, background=SKY, global_scene=g)
        assert (bits(rad_a) == bits(rad_b)).all()
        hits = same_queries(a, b, rays, global_scene=g)
        assert np.isfinite(hits[:, 0]).any() and np.isinf(hits[:, 0]).any()  # the rays cover scene and sky
        assert same_render(render(a, cam, global_scene=g), render(b, cam, global_scene=g))
        va = art.render_views(a, cams, W, H, SPP, seed=9, background=SKY, accum=True, global_scene=g)
        vb = art.render_views(b, cams, W, H, SPP, seed=9, background=SKY, accum=True, global_scene=g)
        assert (va[0] == vb[0]).all() and (bits(va[1]) == bits(vb[1])).all() and va[0].max() > 0
        ga, gb = engine_for(a, cam, global_scene=g).render_guides(), engine_for(b, cam, global_scene=g).render_guides()
        assert ga.shape[-1] == 10 and (bits(ga) == bits(gb)).all()  # all 10 doubles, albedo included
    return ra


# ------------------------------------------------------------------------------------------------ 1. equality with the fresh compile
@pytest.mark.parametrize("name", ["image", "mixed"])
def test_an_updated_scene_equals_the_fresh_compile_of_its_values(gpu, name):
    a, b, cam, before, image_before = updated_pair(name)
    ra = check_pair(a, b, cam, name)
    assert not same_render(ra, before) and ra[0].max() > 0  # the update is visible
    assert kernel_of(ra[2]) == kernel_of(before[2])         # A runs what it ran
    if name == "image":
        assert ra[2]["extend_variant"] == 3 and ra[2]["kernel_lds_mode"] == 3 and image_before is not None
    else:
        assert image_before is None and ra[2]["extend_variant"] != 3


def test_an_unmerged_mixed_world_equals_the_fresh_compile(gpu, options):
    options("compile.world_merge", 0)  # the world stays a list: loose objects, the medium and the BVH side by side
    M0, Md, T0, Td, M1, T1 = values("mixed")
    a, cam = build_mixed(M0, T0), frame_camera("mixed")
    before = render(a, cam)
    art.update_textures(a, T1)
    art.update_materials(a, M1)
    ra = check_pair(a, build_mixed(M1, T1), cam, "mixed")
    assert not same_render(ra, before) and kernel_of(ra[2]) == kernel_of(before[2])


@pytest.mark.parametrize("form", [{"wavefront": True}, {"split_shade": True}, {"global_scene": True}, {"wavefront": True, "global_scene": True}])
def test_every_engine_form_of_the_image_scene_sees_the_update(gpu, form):
    a, b, cam, before, _ = updated_pair("image")
    ra, rb = render(a, cam, **form), render(b, cam, **form)
    assert same_render(ra, rb), (form, int((ra[0] != rb[0]).sum()))
    assert same_render(ra, render(a, cam)) and not same_render(ra, before)  # every form computes the same frame


def test_tile_lists_and_noise_target_of_the_image_scene_follow_the_update(gpu, options):
    a, b, cam, before, _ = updated_pair("image")
    options("render.tile_lists", 2)
    ra, rb = render(a, cam), render(b, cam)
    assert same_render(ra, rb) and ra[2]["extend_variant"] == 3 and not same_render(ra, before)
    ta, tb = engine_for(a, cam).tile_candidates(), engine_for(b, cam).tile_candidates()
    assert ta is not None and (ta == tb).all() and ta.sum() > 0
    options("render.tile_lists", 0)
    assert same_render(render(a, cam), ra)  # the lists change no bit
    outs = []
    for world in (a, b):
        img, acc, cnt = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.float64), np.zeros((H, W), np.int32)
        engine_for(world, cam).run_noise_target(img, accum=acc, counts=cnt, min_spp=4, step_spp=4)
        outs.append((img, acc, cnt))
    assert (outs[0][0] == outs[1][0]).all() and (bits(outs[0][1]) == bits(outs[1][1])).all() and (outs[0][2] == outs[1][2]).all()


# ------------------------------------------------------------------------------------------------ 2. each derived copy on its own
def both_ways(a, b, cam):
    """The frame from the scene's own kernel and from the global records (RT_GLOBAL_SCENE: MatRec.albedo of MATF_SOLID)."""
    for g in (False, True):
        ra, rb = render(a, cam, global_scene=g), render(b, cam, global_scene=g)
        assert same_render(ra, rb), (g, int((ra[0] != rb[0]).sum()))
    return ra


@pytest.mark.parametrize("name", ["image", "mixed"])
def test_the_shared_solid_colour_alone_reaches_the_lambertian_the_light_and_the_checker(gpu, name):
    M0, Md, T0, Td, M1, T1 = values(name)
    a, cam = BUILD[name](M0, T0), frame_camera(name)
    before = render(a, cam)
    sid = a.shared_id
    users = [k for k, (ty, t) in enumerate(Md) if t == sid]
    assert sorted(Md[users, 0]) == [LAMBERTIAN, LIGHT] and sid in [e for ty, e, o in Td if ty == CHECKER]
    art.update_textures(a, np.ascontiguousarray(T1[sid:sid + 1]), first=sid)  # n = 1: every dependent lies outside the range
    mix = np.array(T0)
    mix[sid] = T1[sid]
    ra = both_ways(a, BUILD[name](M0, mix), cam)
    assert not same_render(ra, before)
    assert (bits(art.scene_textures(a)[0]) == bits(mix)).all()


@pytest.mark.parametrize("name", ["image", "mixed"])
def test_the_metals_alone_through_a_sub_range_and_the_clamped_one_alone(gpu, name):
    M0, Md, T0, Td, M1, T1 = values(name)
    a, cam = BUILD[name](M0, T0), frame_camera(name)
    before = render(a, cam)
    metals = np.flatnonzero(Md[:, 0] == METAL)
    first, last = int(metals[0]), int(metals[-1])
    assert last - first + 1 > len(metals) >= 2  # the range holds other materials too: they take nothing
    ty = Md[first:last + 1, 0]
    sub = np.array(M0[first:last + 1])                       # a dielectric in the range takes the ir it has
    sub[ty == METAL, :4], sub[ty == METAL, 4] = M1[first:last + 1][ty == METAL, :4], 99.0  # a metal ignores ir
    sub[(ty == LAMBERTIAN) | (ty == LIGHT)] = 99.0            # ... and these whatever their rows hold
    assert (ty == DIELECTRIC).any() and ((ty == LAMBERTIAN) | (ty == LIGHT)).any()
    art.update_materials(a, sub, first=first)
    mix = np.array(M0)
    mix[metals, :4] = M1[metals, :4]
    ra = both_ways(a, BUILD[name](mix, T0), cam)
    assert not same_render(ra, before)
    assert (bits(art.scene_materials(a)[0]) == bits(held(mix))).all()
    # the fuzz-1.5 metal alone, on a fresh scene: it behaves as fuzz 1
    c, rough = BUILD[name](M0, T0), last
    assert M1[rough, 3] == 1.5
    art.update_materials(c, np.ascontiguousarray(M1[rough:rough + 1]), first=rough)
    one = np.array(M0)
    one[rough, :4] = M1[rough, :4]
    rc = both_ways(c, BUILD[name](one, T0), cam)
    assert not same_render(rc, before)
    one[rough, 3] = 1.0
    assert same_render(rc, render(BUILD[name](one, T0), cam))
    assert art.scene_materials(c)[0][rough, 3] == 1.0


# ------------------------------------------------------------------------------------------------ 3. the image, byte for byte
def test_the_image_is_the_host_builders_byte_for_byte(gpu):
    M0, Md, T0, Td, M1, T1 = values("image")
    a, cam = build_image(M0, T0), frame_camera("image")
    img0 = art.scene_lds_image(a)
    assert img0 is not None and (img0 == art.scene_lds_image(a, rebuilt=True)).all()
    art.update_materials(a, M1)
    art.update_textures(a, T1)
    img1, re1 = art.scene_lds_image(a), art.scene_lds_image(a, rebuilt=True)
    assert (img1 == re1).all(), np.flatnonzero(img1 != re1)[:8]
    assert (img1 == art.scene_lds_image(build_image(M1, T1))).all()  # values alone decide no slot: the fresh compile's image
    changed = np.flatnonzero(img1 != img0)
    assert len(changed) > 100 and changed.min() >= OFF_MAT and changed.max() < OFF_INVR  # the shading table alone
    # 10 entries: ground, shared, checker (2), metal, glass, light, light over shared, metal, glass
    assert not img1[OFF_MAT + 10 * 32:OFF_INVR].any()
    frame1 = render(a, cam)
    # to the values already held: no byte, no frame
    M_now, T_now = art.scene_materials(a)[0], art.scene_textures(a)[0]
    art.update_materials(a, M_now)
    art.update_textures(a, T_now)
    assert (art.scene_lds_image(a) == img1).all() and same_render(render(a, cam), frame1)
    # a second, partial update: the sphere materials' textures back to V0, the second half of the materials to a third set
    M2, T2 = v1(M0, Md, T0, Td, seed=43)
    half = len(M0) // 2
    art.update_materials(a, np.ascontiguousarray(M2[half:]), first=half)
    art.update_textures(a, np.ascontiguousarray(T0[1:4]), first=1)
    img2, re2 = art.scene_lds_image(a), art.scene_lds_image(a, rebuilt=True)
    assert (img2 == re2).all(), np.flatnonzero(img2 != re2)[:8]
    changed = np.flatnonzero(img2 != img1)
    assert len(changed) > 40 and changed.min() >= OFF_MAT and changed.max() < OFF_INVR
    Mmix, Tmix = np.array(M1), np.array(T1)
    Mmix[half:], Tmix[1:4] = M2[half:], T0[1:4]
    fresh = build_image(Mmix, Tmix)
    assert (img2 == art.scene_lds_image(fresh)).all() and same_render(render(a, cam), render(fresh, cam))


# ------------------------------------------------------------------------------------------------ 4. getters and files
@pytest.mark.parametrize("name", ["image", "mixed"])
def test_getters_and_files_follow_the_update(gpu, name, tmp_path):
    M0, Md, T0, Td, M1, T1 = values(name)
    a, b, cam, before, _ = updated_pair(name)
    (Ma, Mda), (Ta, Tda) = art.scene_materials(a), art.scene_textures(a)
    assert (bits(Ma) == bits(held(M1))).all() and (bits(Ta) == bits(T1)).all()  # the clamp applied, ignored fields as before
    assert (Mda == Md).all() and (Tda == Td).all()
    assert Ma[:, 3].max() == 1.0 and (bits(Ma[Md[:, 0] != METAL, :4]) == bits(M0[Md[:, 0] != METAL, :4])).all()
    (Mb, _), (Tb, _) = art.scene_materials(b), art.scene_textures(b)
    assert (bits(Ma) == bits(Mb)).all() and (bits(Ta) == bits(Tb)).all()
    # get -> update is the identity
    frame = render(a, cam)
    art.update_materials(a, Ma)
    art.update_textures(a, Ta)
    assert same_render(render(a, cam), frame)
    assert (bits(art.scene_materials(a)[0]) == bits(Ma)).all() and (bits(art.scene_textures(a)[0]) == bits(Ta)).all()
    # saved and loaded, it renders as the updated one
    path = tmp_path / "updated.art"
    art.save_scene(a, path)
    loaded = art.scene_manager(ASSETS).load(path)
    got = render(loaded.objects, cam)
    assert same_render(got, render(b, cam)) and kernel_of(got[2]) == kernel_of(frame[2])
    assert (bits(art.scene_materials(loaded)[0]) == bits(Ma)).all()
    # the graph no longer describes the updated scene
    assert lib.rt_scene_dump(a._native, None, 0) == 0 and b"updated" in lib.rt_last_error()
    assert lib.rt_scene_dump(b._native, None, 0) > 0


# ------------------------------------------------------------------------------------------------ 5. streams
@pytest.mark.parametrize("name", ["image", "mixed"])
def test_device_tensors_on_a_side_stream_then_views_on_that_stream(gpu, name):
    import torch
    M0, Md, T0, Td, M1, T1 = values(name)
    a, b = BUILD[name](M0, T0), updated_pair(name)[1]
    cams = [frame_camera(name), frame_camera("side"), frame_camera("mixed" if name == "image" else "image")]
    want, want_sums = art.render_views(b, cams, W, H, SPP, seed=9, background=SKY, accum=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        m, t = torch.from_numpy(np.array(M1)).to("cuda"), torch.from_numpy(np.array(T1)).to("cuda")
        assert art.update_materials(a, m) is None and art.update_textures(a, t) is None  # enqueued on the side stream
        got = torch.zeros((3, H, W, 3), dtype=torch.uint8, device="cuda")
        sums = torch.zeros((3, H, W, 3), dtype=torch.float64, device="cuda")
        art.render_views(a, cams, W, H, SPP, seed=9, background=SKY, out=got, accum=sums)
    side.synchronize()
    assert (got.cpu().numpy() == want).all() and (bits(sums.cpu().numpy()) == bits(want_sums)).all()
    assert want.max() > 0


def test_timing_and_the_empty_update(gpu):
    import torch
    M0, Md, T0, Td, M1, T1 = values("image")
    a, cam = build_image(M0, T0), frame_camera("image")
    before = render(a, cam)
    assert art.update_materials(a, np.zeros((0, 5))) is None and art.update_textures(a, np.zeros((0, 4)), first=len(T0)) is None
    assert art.update_materials(a, np.zeros((0, 5)), timing=True) == 0.0
    assert same_render(render(a, cam), before)
    assert lib.rt_scene_dump(a._native, None, 0) > 0  # n = 0 touched nothing: the scene is not an updated one
    ms_m = art.update_materials(a, M1, timing=True)
    ms_t = art.update_textures(a, torch.from_numpy(np.array(T1)).to("cuda"), timing=True)
    assert np.isfinite(ms_m) and ms_m > 0 and np.isfinite(ms_t) and ms_t > 0
    assert same_render(render(a, cam), render(updated_pair("image")[1], cam))


# ------------------------------------------------------------------------------------------------ 6. combined with geometry
def jitter(s0, seed=31):
    rng = np.random.default_rng(seed)
    s = np.array(s0)
    small = s0[:, 3] < 10.0
    s[small, :3] += rng.uniform(-1.0, 1.0, (int(small.sum()), 3)) * s0[small, 3:4]
    s[small, 3] *= rng.uniform(0.7, 1.3, int(small.sum()))
    return quant(s)


@pytest.mark.parametrize("spheres_first", [True, False])
def test_sphere_and_texture_updates_combine_in_either_order(gpu, spheres_first):
    M0, Md, T0, Td, M1, T1 = values("image")
    a, cam = build_image(M0, T0), frame_camera("image")
    s1 = jitter(IMAGE_S0)
    steps = [lambda: art.update_spheres(a, s1), lambda: art.update_textures(a, T1)]
    for step in steps if spheres_first else steps[::-1]:
        step()
    b = build_image(M0, T1, s1)
    assert same_render(render(a, cam), render(b, cam))
    assert same_render(render(a, cam, global_scene=True), render(b, cam, global_scene=True))
    assert (art.scene_lds_image(a) == art.scene_lds_image(a, rebuilt=True)).all()
    assert not same_render(render(a, cam), render(build_image(M0, T1), cam))  # the spheres did move


# ------------------------------------------------------------------------------------------------ 7. builtin scenes
@pytest.mark.parametrize("scene", ["cow", "1"])
def test_a_builtin_scene_survives_a_round_trip_of_its_values(gpu, scene):
    # cow: one lambertian per triangle from color::random(); scene 1 (the benchmark scene): an image with hundreds of entries
    sm = art.scene_manager(ASSETS)
    world, untouched = sm.build(scene), sm.build(scene)
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    ref = render(untouched.objects, cam, world.background)
    (M0, Md), (T0, Td) = art.scene_materials(world), art.scene_textures(world)
    assert len(M0) == world.info["materials"] and len(T0) == world.info["textures"] and (Td[:, 0] == SOLID).sum() > 100
    image0 = art.scene_lds_image(world)
    M1, T1 = np.array(M0), np.array(T0)
    rng = np.random.default_rng(51)
    T1[Td[:, 0] == SOLID, :3] = rng.uniform(0.05, 0.95, (int((Td[:, 0] == SOLID).sum()), 3))
    art.update_textures(world, T1)
    if scene == "1":
        metal, glass = Md[:, 0] == METAL, Md[:, 0] == DIELECTRIC
        assert image0 is not None and metal.sum() > 10 and glass.sum() > 3
        M1[metal, :4] = rng.uniform(0.0, 0.9, (int(metal.sum()), 4))
        M1[glass, 4] = rng.uniform(1.2, 2.4, int(glass.sum()))
        art.update_materials(world, M1)
        image1 = art.scene_lds_image(world)
        assert (image1 == art.scene_lds_image(world, rebuilt=True)).all()
        changed = np.flatnonzero(image1 != image0)
        assert len(changed) > 3000 and changed.min() >= OFF_MAT and changed.max() < OFF_INVR
    up = render(world.objects, cam, world.background)
    assert not same_render(up, ref) and kernel_of(up[2]) == kernel_of(ref[2])
    assert (bits(art.scene_textures(world)[0]) == bits(T1)).all() and (bits(art.scene_materials(world)[0]) == bits(M1)).all()
    art.update_textures(world, T0)
    art.update_materials(world, M0)
    back = render(world.objects, cam, world.background)
    assert same_render(back, ref) and kernel_of(back[2]) == kernel_of(ref[2])
    assert (bits(art.scene_textures(world)[0]) == bits(T0)).all() and (bits(art.scene_materials(world)[0]) == bits(M0)).all()
    if scene == "1":
        assert (art.scene_lds_image(world) == image0).all() and back[2]["extend_variant"] == 3
