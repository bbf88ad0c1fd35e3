"""rt_radiance_grad_texels and rt_scene_update_texels on the GPU.  Closed forms on small caller-built scenes (67 rays: a
wave and three) with the texel of every ray from a host restatement of image_value's index arithmetic; the other
outputs against rt_radiance_grad's bits; central differences through update_texels at max_depth 3, where phi has degree
<= 2 in the texel values; bits that depend on neither the order of the rays, the buffers' place, the texel table's copy
count nor the kernel form; update_texels against a fresh compile; the Python layers; the workspace fault point."""
import functools
import math

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd.rays import _native_scene
from tests.update_common import SKY, bits, engine_for, frame_camera, render, same_render

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 32, 18, 4, 3
NP = W * H * SPP
EPS = 2.0 ** -52
N = 67
BG = (1.0, 0.5, 0.25)
CS = 1.0 / 255.0  # image_value's colour scale: a texel's value is CS * byte, rounded once


# ------------------------------------------------------------------------------------------------ helpers
def texel_index(u, v, w, h):
    """image_value's index arithmetic (device.h, texture.h:90-117) restated: (i, j) of the texel u, v read."""
    u = np.minimum(np.maximum(np.asarray(u, np.float64), 0.0), 1.0)
    v = 1.0 - np.minimum(np.maximum(np.asarray(v, np.float64), 0.0), 1.0)
    i = np.minimum((u * float(w)).astype(np.int64), w - 1)  # a cast truncates towards zero; both are >= 0
    j = np.minimum((v * float(h)).astype(np.int64), h - 1)
    return i, j


def values_of(px):
    """The three channel values of every texel of an (h, w, bpp) byte image, (h * w, 3)."""
    return (CS * px[:, :, :3].astype(np.float64)).reshape(-1, 3)


def exact_rows(n_rows, rows, terms, repeat=1):
    """out[r] = the correctly rounded exact sum of `repeat` copies of the terms whose row is r (what the integer
    accumulators give: no term here is below their 2^-96 quantum); every other row +0.0."""
    out = np.zeros((n_rows, 3))
    for r in np.unique(rows):
        mine = terms[rows == r]
        for c in range(3):
            out[r, c] = math.fsum(list(mine[:, c]) * repeat)
    return out


def in_order(term, spp):
    acc = np.zeros_like(term)
    for _ in range(spp):
        acc = acc + term
    return acc


def dyadic_weights(n, seed):
    return np.random.default_rng(seed).integers(-16, 17, (n, 3)) / 8.0


def image_bytes(h, w, bpp, seed):
    """Bytes in [16, 239]: a move of +-8 stays a byte, and every value is well above zero."""
    return np.random.default_rng(seed).integers(16, 240, (h, w, bpp)).astype(np.uint8)


def compiled(w):
    return art.hittable_list(native=art.compile_world(w, 0))


def down_rays(x, y):
    """Rays from z = 5 straight down -z through (x, y)."""
    n = len(x)
    return np.ascontiguousarray(np.stack([x, y, np.full(n, 5.0), np.zeros(n), np.zeros(n), np.full(n, -1.0), np.zeros(n)], axis=1))


def interior_points(rnd, n, x0, x1, y0, y1, w, h):
    """n points of [x0, x1] x [y0, y1], each at least a tenth of a texel away from the border of its texel of a w x h image
    over the rectangle: the texel does not hang on the last bit of u or v."""
    ti, tj = rnd.integers(0, w, n), rnd.integers(0, h, n)
    x = x0 + (ti + rnd.uniform(0.1, 0.9, n)) * (x1 - x0) / w
    y = y0 + (tj + rnd.uniform(0.1, 0.9, n)) * (y1 - y0) / h
    return x, y


IMG_A, IMG_B, IMG_C = image_bytes(3, 4, 3, 1), image_bytes(2, 5, 4, 2), image_bytes(2, 2, 3, 3)
RECT_A, RECT_B = (0.0, 4.0, 0.0, 3.0), (10.0, 15.0, 0.0, 2.0)


def two_rects(a=IMG_A, b=IMG_B, light=False):
    """Two coplanar xy rects, image A (4 x 3, bpp 3) on the first and image B (5 x 2, bpp 4) on the second, as lambertians
    or as lights; a third image (2 x 2) that no object uses.  A ray scattered off one rect can hit neither."""
    art.reset_scene_rng()
    w = art.hittable_list()
    mat = art.diffuse_light if light else art.lambertian
    w.add(art.xy_rect(*RECT_A, 0.0, mat(art.image_texture(a))))
    w.add(art.xy_rect(*RECT_B, 0.0, mat(art.image_texture(b))))
    art.image_texture(IMG_C)
    return compiled(w)


@functools.lru_cache(maxsize=None)
def rect_world(light=False):
    return two_rects(light=light)


def rect_case(which, seed):
    """67 rays aimed at rect A, rect B or both, with each ray's global texel and value."""
    rnd = np.random.default_rng(seed)
    on_b = {"A": np.zeros(N, bool), "B": np.ones(N, bool), "both": rnd.random(N) < 0.5}[which]
    xa, ya = interior_points(rnd, N, *RECT_A, 4, 3)
    xb, yb = interior_points(rnd, N, *RECT_B, 5, 2)
    x, y = np.where(on_b, xb, xa), np.where(on_b, yb, ya)
    ua, va = (x - RECT_A[0]) / (RECT_A[1] - RECT_A[0]), (y - RECT_A[2]) / (RECT_A[3] - RECT_A[2])
    ub, vb = (x - RECT_B[0]) / (RECT_B[1] - RECT_B[0]), (y - RECT_B[2]) / (RECT_B[3] - RECT_B[2])
    ia, ja = texel_index(ua, va, 4, 3)
    ib, jb = texel_index(ub, vb, 5, 2)
    texel = np.where(on_b, 12 + jb * 5 + ib, ja * 4 + ia)   # first_B = 4 * 3
    value = np.where(on_b[:, None], values_of(IMG_B)[jb * 5 + ib], values_of(IMG_A)[ja * 4 + ia])
    return down_rays(x, y), texel, value


# ------------------------------------------------------------------------------------------------ 1. closed form, lambertian
@pytest.mark.parametrize("which", ["A", "B", "both"])
def test_one_lambertian_bounce_off_an_image_gives_the_products_exactly(gpu, which):
    world = rect_world()
    desc, first, _ = art.scene_images(world)
    assert desc.tolist() == [[4, 3, 3], [5, 2, 4], [2, 2, 3]] and first.tolist() == [0, 12, 22]
    rays, texel, value = rect_case(which, 5)
    spp, w, bg = 8, dyadic_weights(N, 6), np.array(BG)
    L, gt, gm, gb, gx, st = art.radiance_grad(world, rays, w, spp=spp, max_depth=2, background=BG, seed=1, stats=True, texels=True)
    assert st["segments"] == 2 * N * spp  # every path: the rect, then the sky
    assert (bits(L) == bits(in_order(value * bg, spp))).all()
    assert gx.shape == (26, 3)
    # vertex 0 adds (w * P_0) * Q_0 = w * background to its texel's row; the end adds w * P_1 = w * value to the background's
    assert (bits(gx) == bits(exact_rows(26, texel, w * bg, spp))).all()
    assert (bits(gb) == bits(exact_rows(1, np.zeros(N, int), w * value, spp)[0])).all()
    assert (bits(gt) == 0).all() and (bits(gm) == 0).all()
    assert (bits(gx[22:]) == 0).all()            # the image nothing uses
    if which == "A":
        assert (bits(gx[12:]) == 0).all() and np.abs(gx[:12]).max() > 0.0
    if which == "B":
        assert (bits(gx[:12]) == 0).all() and np.abs(gx[12:22]).max() > 0.0  # first_k != 0, bpp 4


# ------------------------------------------------------------------------------------------------ 2. image emitters
def test_an_image_light_hit_directly_adds_the_weight_to_its_texel(gpu):
    world = rect_world(light=True)
    rays, texel, value = rect_case("both", 7)
    spp, w = 8, dyadic_weights(N, 8)
    L, gt, gm, gb, gx = art.radiance_grad(world, rays, w, spp=spp, max_depth=4, background=BG, seed=2, texels=True)
    assert (bits(L) == bits(in_order(value, spp))).all()
    assert (bits(gx) == bits(exact_rows(26, texel, w, spp))).all()   # the end adds w * P_0 = w
    assert (bits(gb) == 0).all() and (bits(gt) == 0).all()


@functools.lru_cache(maxsize=None)
def lamp_world():
    """An image light (8 x 4) above a solid lambertian floor and sphere, beside a solid light: texels are emission only."""
    art.reset_scene_rng()
    w = art.hittable_list()
    w.add(art.xz_rect(-2.0, 2.0, -2.0, 2.0, 3.0, art.diffuse_light(art.image_texture(image_bytes(4, 8, 3, 4)))))
    w.add(art.xz_rect(-6.0, 6.0, -6.0, 6.0, 0.0, art.lambertian(art.solid_color(0.75, 0.5, 0.25))))
    w.add(art.sphere((0.0, 1.0, 0.0), 1.0, art.lambertian(art.solid_color(0.25, 0.5, 0.75))))
    w.add(art.sphere((3.0, 1.0, 0.0), 0.5, art.diffuse_light(art.solid_color(2.0, 1.0, 4.0))))
    return compiled(w)


def lamp_rays(n=NP):
    rnd = np.random.default_rng(9)
    o = np.array([0.0, 2.0, 8.0]) + rnd.uniform(-0.5, 0.5, (n, 3))
    target = np.stack([rnd.uniform(-3.5, 3.5, n), rnd.uniform(0.0, 3.2, n), rnd.uniform(-2.0, 2.0, n)], axis=1)
    return np.ascontiguousarray(np.concatenate([o, target - o, np.zeros((n, 1))], axis=1))


def test_eulers_identity_over_emitter_rows_texel_rows_and_the_background(gpu):
    world, rays, depth = lamp_world(), lamp_rays(), 12
    w = np.random.default_rng(10).uniform(0.25, 1.0, (NP, 3))
    L, gt, gm, gb, gx = art.radiance_grad(world, rays, w, spp=1, max_depth=depth, background=BG, seed=3, texels=True)
    T, td = art.scene_textures(world)
    emit = 3  # the solid light's texture: image 0, the two lambertian colours 1 and 2, then the lamp's
    assert td[emit, 0] == 0 and (T[emit, :3] == (2.0, 1.0, 4.0)).all()
    lhs = math.fsum((gx * values_of(art.scene_texels(world, 0))).ravel()) + math.fsum(gt[emit, :3] * T[emit, :3]) + math.fsum(gb * np.array(BG))
    rhs = math.fsum((w * L).ravel())
    print(f"emitters, texels and background {lhs!r} radiance {rhs!r} gap {abs(lhs - rhs):.3e} bound {4.0 * NP * depth * EPS * rhs:.3e}")
    assert rhs > 0.0 and np.abs(gx).max() > 0.0 and np.abs(gt[emit]).max() > 0.0
    assert abs(lhs - rhs) <= 4.0 * NP * depth * EPS * rhs


# ------------------------------------------------------------------------------------------------ 3. through get_sphere_uv
def test_a_texel_through_the_spheres_uv(gpu):
    art.reset_scene_rng()
    px = image_bytes(4, 8, 3, 11)
    wl = art.hittable_list()
    wl.add(art.sphere((0.0, 0.0, 0.0), 1.0, art.lambertian(art.image_texture(px))))
    world = compiled(wl)
    rnd = np.random.default_rng(12)
    o = rnd.normal(size=(N, 3))
    o = 5.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    rays = np.ascontiguousarray(np.concatenate([o, rnd.uniform(-0.5, 0.5, (N, 3)) - o, np.zeros((N, 1))], axis=1))
    hits = art.query_rays(world, rays).records
    assert np.isfinite(hits[:, 0]).all()
    i, j = texel_index(hits[:, 7], hits[:, 8], 8, 4)
    texel, value = j * 8 + i, values_of(px)[j * 8 + i]
    assert len(np.unique(texel)) > 8
    spp, w, bg = 8, dyadic_weights(N, 13), np.array(BG)
    L, gt, gm, gb, gx = art.radiance_grad(world, rays, w, spp=spp, max_depth=2, background=BG, seed=4, texels=True)
    assert (bits(L) == bits(in_order(value * bg, spp))).all()   # a ray scattered off a sphere cannot hit it again
    assert (bits(gx) == bits(exact_rows(32, texel, w * bg, spp))).all()
    assert (bits(gb) == bits(exact_rows(1, np.zeros(N, int), w * value, spp)[0])).all()


# ------------------------------------------------------------------------------------------------ 4. barycentric image
def test_a_barycentric_image_over_two_triangles(gpu):
    art.reset_scene_rng()
    px = image_bytes(4, 4, 3, 14)
    img = art.image_texture(px)
    quad = [(0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (4.0, 4.0, 0.0), (0.0, 4.0, 0.0)]
    uvq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
    wl = art.hittable_list()
    corners = [(0, 1, 2), (0, 2, 3)]
    for a, b, c in corners:
        wl.add(art.triangle(quad[a], quad[b], quad[c], art.lambertian(art.barycentric_image_texture(uvq[a], uvq[b], uvq[c], img))))
    world = compiled(wl)
    rnd = np.random.default_rng(15)
    x, y = interior_points(rnd, N, 0.0, 4.0, 0.0, 4.0, 4, 4)
    rays = down_rays(x, y)
    hits = art.query_rays(world, rays).records
    assert np.isfinite(hits[:, 0]).all()
    u, v, prim = hits[:, 7], hits[:, 8], hits[:, 10].astype(np.int64) & ((1 << 30) - 1)  # the reference's index under its type bits
    assert set(prim) == {0, 1}
    uv = np.array([[*uvq[a], *uvq[b], *uvq[c]] for a, b, c in corners])[prim]   # the texture's texcoords a, b, c per ray
    wb = 1.0 - u - v
    iu = u * uv[:, 0] + v * uv[:, 2] + wb * uv[:, 4]                             # tex_value's products, in its order
    iv = u * uv[:, 1] + v * uv[:, 3] + wb * uv[:, 5]
    i, j = texel_index(iu, iv, 4, 4)
    texel, value = j * 4 + i, values_of(px)[j * 4 + i]
    assert len(np.unique(texel)) > 8
    spp, w, bg = 8, dyadic_weights(N, 16), np.array(BG)
    L, gt, gm, gb, gx = art.radiance_grad(world, rays, w, spp=spp, max_depth=2, background=BG, seed=5, texels=True)
    assert (bits(L) == bits(in_order(value * bg, spp))).all()
    assert (bits(gx) == bits(exact_rows(16, texel, w * bg, spp))).all()
    assert (bits(gb) == bits(exact_rows(1, np.zeros(N, int), w * value, spp)[0])).all()


# ------------------------------------------------------------------------------------------------ 5. the rest is rt_radiance_grad
@functools.lru_cache(maxsize=None)
def world_of(scene):
    return art.scene_manager().build(scene)


def camera_of(world, w, h):
    return art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, w / h, world.aperture, 10.0, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def paths_of(scene):
    rays, rng = art.camera_rays(camera_of(world_of(scene), W, H), W, H, SPP, seed=SEED)
    rays.setflags(write=False)
    rng.setflags(write=False)
    return rays, rng


@functools.lru_cache(maxsize=None)
def weights_of(kind):
    rnd = np.random.default_rng(11)
    w = rnd.uniform(0.25, 1.0, (NP, 3)) if kind == "positive" else rnd.uniform(-1.0, 1.0, (NP, 3))
    w.setflags(write=False)
    return w


def grad_of(scene, kind, max_depth, **kw):
    rays, rng = paths_of(scene)
    return art.radiance_grad(world_of(scene), rays, weights_of(kind), rng=rng, spp=1, max_depth=max_depth, texels=True, **kw)


def same(a, b):
    return len(a) == len(b) and all((bits(x) == bits(y)).all() for x, y in zip(a, b))


@pytest.mark.parametrize("scene", ["4", "8", "9"])
def test_every_other_output_is_rt_radiance_grads(gpu, scene):
    rays, rng = paths_of(scene)
    want, st = art.radiance_rays(world_of(scene), rays, rng=rng, spp=1, stats=True)
    plain = art.radiance_grad(world_of(scene), rays, weights_of("signed"), rng=rng, spp=1, max_depth=50)
    L, gt, gm, gb, gx, gst = grad_of(scene, "signed", 50, stats=True)
    assert (bits(L) == bits(want)).all() and gst["segments"] == st["segments"] and gst["primary"] == NP
    assert same((L, gt, gm, gb), plain)
    desc, first, _ = art.scene_images(world_of(scene))
    assert gx.shape == (int((desc[:, 0].astype(np.int64) * desc[:, 1]).sum()), 3)
    assert np.isfinite(gx).all() and np.abs(gx).max() > 0.0
    assert (bits(gx) != 0).any(1).sum() <= 50 * NP  # a path reads a texel per vertex at most: the rest is +0.0


# ------------------------------------------------------------------------------------------------ 6. central differences
def texel_difference(world, image, radiance, w, depth, gx, first):
    """(phi+ - phi-) / 2h through update_texels (every byte of the image's first three channels in [8, 247] moved by +-8,
    h = 8 / 255; radiance(): radiance_rays on the call's paths), <grad, d> with d = (v+ - v-) / 2h restated from the
    bytes, and the rounding bound; the bytes are put back."""
    b0 = art.scene_texels(world, image)
    moved = np.zeros(b0.shape, bool)
    moved[:, :, :3] = (b0[:, :, :3] >= 8) & (b0[:, :, :3] <= 247)
    h = 8.0 / 255.0
    vals, bound, v = [], 0.0, []
    try:
        for sign in (8, -8):
            b = np.where(moved, b0.astype(np.int64) + sign, b0).astype(np.uint8)
            art.update_texels(world, image, b)
            L = radiance()
            vals.append(math.fsum((w * L).ravel()))
            v.append(values_of(b))
            # fd_bound of tests/test_gpu_radiance_grad.py with 2 * max_depth factors: each texel factor carries CS * byte's own rounding
            bound = max(bound, 4.0 * len(w) * (2 * depth) * EPS * float((np.abs(w) * np.abs(L)).sum()) / h)
    finally:
        art.update_texels(world, image, b0)
    d = (v[0] - v[1]) / (2.0 * h)
    rows = gx[first:first + len(d)]
    assert (d >= 0.0).all() and (rows >= 0.0).all() and moved.any()  # every term of <grad, d> is positive or zero: none cancels
    read = rows != 0.0  # (most texels of a large image: no path read them)
    return (vals[0] - vals[1]) / (2.0 * h), math.fsum(rows[read] * d[read]), bound


@pytest.mark.parametrize("scene", ["4", "9", "lamp"])
def test_central_differences_through_update_texels_are_exact_at_depth_three(gpu, scene):
    """At max_depth 3 a path has at most two scatter vertices and an end: phi has degree <= 2 in the texel values (1
    where they are emission), so the central difference has no truncation error and differs from <grad, d> by rounding
    alone.  The weights are positive and every byte moves the same way, so no term of <grad, d> cancels another."""
    depth = 3
    if scene == "lamp":  # the image light: paths keyed by the seed
        world, rays, w = lamp_world(), lamp_rays(), np.random.default_rng(10).uniform(0.25, 1.0, (NP, 3))
        kw = dict(spp=1, max_depth=depth, background=BG, seed=3)
    else:
        world, (rays, rng), w = world_of(scene), paths_of(scene), weights_of("positive")
        kw = dict(spp=1, max_depth=depth, rng=rng)
    gx = art.radiance_grad(world, rays, w, texels=True, **kw)[4]
    _, first, _ = art.scene_images(world)
    fd, slope, bound = texel_difference(world, 0, lambda: art.radiance_rays(world, rays, **kw), w, depth, gx, int(first[0]))
    print(f"scene {scene}: <grad, d> {slope!r} central difference {fd!r} gap {abs(slope - fd):.3e} bound {bound:.3e}")
    assert slope > 0.0
    assert bound < 1e-2 * abs(slope)
    assert abs(slope - fd) <= bound


# ------------------------------------------------------------------------------------------------ 7. exactness
def test_the_same_call_twice_and_permuted_rays_give_the_same_bits(gpu):
    (rays, rng), w = paths_of("4"), weights_of("signed")
    a, b = grad_of("4", "signed", 50), grad_of("4", "signed", 50)
    assert same(a, b)
    perm = np.random.default_rng(31).permutation(NP)
    c = art.radiance_grad(world_of("4"), np.ascontiguousarray(rays[perm]), np.ascontiguousarray(w[perm]), rng=np.ascontiguousarray(rng[perm]),
                          spp=1, max_depth=50, texels=True)
    assert same(a[1:], c[1:]) and (bits(a[0][perm]) == bits(c[0])).all()


def test_host_buffers_and_device_tensors_on_a_side_stream_agree(gpu):
    import torch
    (rays, rng), w = paths_of("9"), weights_of("signed")
    host = grad_of("9", "signed", 50)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_rays, d_w = torch.from_numpy(np.array(rays)).to("cuda"), torch.from_numpy(np.array(w)).to("cuda")
        d_rng = torch.from_numpy(np.array(rng).view(np.int64)).to("cuda")
        dev = art.radiance_grad(world_of("9"), d_rays, d_w, rng=d_rng, spp=1, max_depth=50, texels=True)  # enqueued on `side`
    assert all(x.is_cuda for x in dev) and len(dev) == 5
    side.synchronize()
    assert same(host, [x.cpu().numpy() for x in dev])


@pytest.mark.parametrize("scene", ["4", "9"])
def test_the_texel_tables_copy_count_changes_no_bit(gpu, options, scene):
    auto = grad_of(scene, "signed", 50)
    options("grad.texel_copies", 1)
    one = grad_of(scene, "signed", 50)
    options("grad.texel_copies", 64)
    most = grad_of(scene, "signed", 50)
    assert same(auto, one) and same(auto, most) and np.abs(auto[4]).max() > 0.0


def test_the_global_scene_flag_changes_no_bit(gpu):
    assert same(grad_of("8", "signed", 50), grad_of("8", "signed", 50, global_scene=True))


def test_a_scene_without_an_image_gets_an_empty_texel_gradient(gpu):
    # scene 1 has no image: the call is rt_radiance_grad's kernel, and grad_texels has no row
    rays, rng = paths_of("1")
    plain = art.radiance_grad(world_of("1"), rays, weights_of("signed"), rng=rng, spp=1, max_depth=8)
    got = art.radiance_grad(world_of("1"), rays, weights_of("signed"), rng=rng, spp=1, max_depth=8, texels=True)
    assert got[4].shape == (0, 3) and same(plain, got[:4])


# ------------------------------------------------------------------------------------------------ 8. update_texels parity
def globe_world(px):
    """Spheres only, so that rt_render runs its LDS-scene kernels: an image-textured ground and globe, a metal and a lamp."""
    art.reset_scene_rng()
    w = art.hittable_list()
    tex = art.image_texture(px)
    w.add(art.sphere((0.0, -100.0, 0.0), 100.0, art.lambertian(tex)))
    w.add(art.sphere((0.0, 1.0, 0.0), 1.0, art.lambertian(tex)))
    w.add(art.sphere((2.2, 0.7, 0.5), 0.7, art.metal((0.8, 0.7, 0.6), 0.1)))
    w.add(art.sphere((-2.0, 0.6, 1.0), 0.6, art.diffuse_light(art.solid_color(3.0, 2.5, 2.0))))
    return compiled(w)


V0, V1 = image_bytes(8, 16, 3, 21), image_bytes(8, 16, 3, 22)


def check_pair(a, b):
    cam = frame_camera("image")
    for form in ({}, {"wavefront": True}, {"global_scene": True}):
        ra, rb = render(a, cam, **form), render(b, cam, **form)
        assert same_render(ra, rb), form
        assert ra[0].max() > 0
    rays, _ = art.camera_rays(cam, 32, 18, 1)
    assert (bits(art.radiance_rays(a, rays, spp=2, seed=3, background=SKY)) == bits(art.radiance_rays(b, rays, spp=2, seed=3, background=SKY))).all()
    ga, gb = engine_for(a, cam).render_guides(), engine_for(b, cam).render_guides()
    assert (bits(ga) == bits(gb)).all()  # all 10 doubles, albedo included
    w = np.random.default_rng(23).uniform(-1.0, 1.0, (len(rays), 3))
    assert same(art.radiance_grad(a, rays, w, spp=2, seed=3, background=SKY, texels=True), art.radiance_grad(b, rays, w, spp=2, seed=3, background=SKY, texels=True))


@pytest.mark.parametrize("how", ["whole", "rows", "tensor"])
def test_an_updated_image_equals_the_fresh_compile_of_its_bytes(gpu, how, tmp_path):
    a, b = globe_world(V0), globe_world(V1)
    before = render(a, frame_camera("image"))
    if how == "whole":
        art.update_texels(a, 0, V1)
    elif how == "rows":
        art.update_texels(a, 0, V1[5:], first_row=5)
        art.update_texels(a, 0, np.ascontiguousarray(V1[:2]))
        assert art.update_texels(a, 0, np.ascontiguousarray(V1[2:5]), first_row=2, timing=True) >= 0.0
    else:
        import torch
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            art.update_texels(a, 0, torch.from_numpy(V1[:4].copy()).to("cuda"))               # enqueued on `side`
            art.update_texels(a, 0, torch.from_numpy(V1[4:].copy()).to("cuda"), first_row=4)
        side.synchronize()
    assert np.array_equal(art.scene_texels(a, 0), V1)
    check_pair(a, b)
    assert not same_render(before, render(a, frame_camera("image")))
    # a save / load round trip holds the new bytes; a get followed by an update changes no bit
    path = tmp_path / "globe.art"
    art.save_scene(a, path)
    loaded = art.scene_manager().load(path)
    assert np.array_equal(art.scene_texels(loaded, 0), V1)
    art.update_texels(a, 0, art.scene_texels(a, 0))
    check_pair(a, b)
    from another_raytracer_amd._lib import lib
    assert lib.rt_scene_dump(_native_scene(a), None, 0) == 0 and b"updated" in lib.rt_last_error()  # an updated scene has no dump


# ------------------------------------------------------------------------------------------------ 9. the Python layers
@pytest.mark.parametrize("place", ["numpy", "cuda"])
def test_render_grad_with_texels_is_radiance_grad_of_the_camera_rays(gpu, place):
    world = world_of("4")
    cam = camera_of(world, W, H)
    adj = np.random.default_rng(51).uniform(-1.0, 1.0, (H, W, 3))
    if place == "numpy":
        out = art.render_grad(world, cam, W, H, SPP, adj, seed=SEED, texels=True)
    else:
        import torch
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            out = art.render_grad(world, cam, W, H, SPP, torch.from_numpy(adj).to("cuda"), seed=SEED, texels=True)
        side.synchronize()
        out = [x.cpu().numpy() for x in out]
    assert len(out) == 5
    rays, rng = paths_of("4")
    want = art.radiance_grad(world, rays, np.ascontiguousarray(np.repeat(adj.reshape(-1, 3), SPP, axis=0)), rng=rng, spp=1, texels=True)
    assert same(out[1:], want[1:]) and np.abs(out[4]).max() > 0.0


@pytest.mark.parametrize("place", ["cpu", "cuda"])
def test_the_autograd_function_hands_back_the_images_rows(gpu, place):
    import torch
    world = two_rects()  # its own copy: the forward pass writes the bytes into the scene
    rays, _, _ = rect_case("both", 5)
    w = dyadic_weights(N, 6)
    t_rays, t_w = torch.from_numpy(rays).to(place), torch.from_numpy(w).to(place)
    xa = torch.from_numpy(IMG_A[:, :, :3] / 255.0).to(place).requires_grad_()
    xb = torch.from_numpy(IMG_B[:, :, :3] / 255.0).to(place).requires_grad_()
    bg = torch.tensor(BG, dtype=torch.float64, device=place)
    L = art.differentiable_radiance(world, t_rays, background=bg, texels={0: xa, 1: xb}, spp=8, max_depth=2, seed=1)
    assert np.array_equal(art.scene_texels(world, 0), IMG_A) and np.array_equal(art.scene_texels(world, 1), IMG_B)  # byte / 255 round-trips
    (L * t_w).sum().backward()
    want = art.radiance_grad(world, rays, w, spp=8, max_depth=2, seed=1, background=BG, texels=True)
    assert (bits(L.detach().cpu().numpy()) == bits(want[0])).all()
    assert (bits(xa.grad.cpu().numpy()) == bits(want[4][:12].reshape(3, 4, 3))).all()
    assert (bits(xb.grad.cpu().numpy()) == bits(want[4][12:22].reshape(2, 5, 3))).all()
    assert xa.grad.device == xa.device and np.abs(want[4]).max() > 0.0


def test_three_descent_steps_towards_a_target_image_lower_the_loss(gpu):
    """The scene of test 1: radiance_i = spp * background * value(texel_i) in every channel, so the loss
    1/2 sum_i |radiance_i - target_i|^2 is a separable quadratic in the texel values with curvature n_t * (spp * bg_c)^2
    for a texel n_t rays read.  A step of half the inverse of the largest curvature halves the fastest coordinate's
    distance to the target and overshoots none; the target is 64 byte steps or more away, so every step changes bytes."""
    import torch
    start = np.where(IMG_A >= 128, IMG_A - 100, IMG_A + 100).astype(np.uint8)   # |start - target| = 100 bytes
    world = two_rects(a=start)
    rays, texel, value = rect_case("A", 5)
    spp, bg = 8, np.array(BG)
    target = torch.from_numpy(in_order(value * bg, spp))
    counts = np.bincount(texel, minlength=12).max()
    lr = 0.5 / (counts * (spp * bg.max()) ** 2)
    x = torch.from_numpy(start[:, :, :3] / 255.0).requires_grad_()
    losses = []
    for _ in range(4):
        L = art.differentiable_radiance(world, torch.from_numpy(rays), background=torch.tensor(BG, dtype=torch.float64), texels={0: x}, spp=spp,
                                        max_depth=2, seed=1)
        loss = 0.5 * ((L - target) ** 2).sum()
        losses.append(float(loss.detach()))
        x.grad = None
        loss.backward()
        with torch.no_grad():
            x -= lr * x.grad
    print("losses", losses)
    assert losses[0] > losses[1] > losses[2] > losses[3] > 0.0


# ------------------------------------------------------------------------------------------------ 10. the workspace fault point
def test_a_refused_workspace_fails_the_call_and_the_next_one_works(gpu, options):
    world = two_rects()  # a scene of its own: its workspace is empty
    rays, _, _ = rect_case("both", 5)
    w = dyadic_weights(N, 6)
    want = art.radiance_grad(rect_world(), rays, w, spp=SPP, seed=4, max_depth=2, background=BG, texels=True)
    options("test.fault_workspace_bytes", 4096)
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.radiance_grad(world, rays, w, spp=SPP, seed=4, max_depth=2, background=BG, texels=True)
    options("test.fault_workspace_bytes", 0)
    got = art.radiance_grad(world, rays, w, spp=SPP, seed=4, max_depth=2, background=BG, texels=True)
    assert same(want, got)
