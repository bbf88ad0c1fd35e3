"""rt_radiance_grad on the GPU.  The path is rt_radiance_rays' (radiance and segments equal in bits); the gradient is
checked against closed forms on a one-sphere scene, against central differences of radiance_rays after update_textures /
update_materials (exact where the radiance has degree <= 2 in the varied colours), against Euler's identity for the
degree-1 emitter colours, and for bits that depend on neither the order of the rays, the buffers' place nor the kernel
form.  32 x 18 camera rays x 4 samples = 2 304 paths unless stated."""
import functools
import math

import numpy as np
import pytest

import another_raytracer_amd as art

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 32, 18, 4, 3
NP = W * H * SPP
EPS = 2.0 ** -52
SOLID, CHECKER = 0, 1
LAMBERTIAN, METAL, DIELECTRIC, LIGHT, ISOTROPIC = range(5)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@functools.lru_cache(maxsize=None)
def world_of(scene):
    return art.scene_manager().build(scene)


def camera_of(world, w, h):
    return art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, w / h, world.aperture, 10.0, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def paths_of(scene):
    """The scene's 2 304 camera rays and post-camera PCG states (one path per ray), read-only."""
    rays, rng = art.camera_rays(camera_of(world_of(scene), W, H), W, H, SPP, seed=SEED)
    rays.setflags(write=False)
    rng.setflags(write=False)
    return rays, rng


@functools.lru_cache(maxsize=None)
def weights_of(kind, n=NP):
    rnd = np.random.default_rng(11)
    w = rnd.uniform(0.25, 1.0, (n, 3)) if kind == "positive" else rnd.uniform(-1.0, 1.0, (n, 3))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def structure(scene):
    """(emitter rows, attenuation rows, metal rows, plain) of a scene: the solid textures its diffuse_lights resolve to
    (through checker levels) and no lambertian or isotropic does, those its lambertians and isotropics resolve to and no
    light does, and its metal materials.  plain: every light's texture tree ends in solid colours and no colour is both an
    emission and an attenuation -- then the radiance has degree 1 in the emitter rows and the background together."""
    _, td = art.scene_textures(world_of(scene))
    _, md = art.scene_materials(world_of(scene))

    def resolve(t, out):
        if td[t, 0] == SOLID:
            out.add(int(t))
            return True
        return td[t, 0] == CHECKER and all([resolve(td[t, 1], out), resolve(td[t, 2], out)])
    emit, att, plain = set(), set(), True
    for ty, tex in md:
        if ty == LIGHT:
            plain = resolve(tex, emit) and plain
        elif ty in (LAMBERTIAN, ISOTROPIC):
            resolve(tex, att)
    plain = plain and not (emit & att)
    return sorted(emit - att), sorted(att - emit), [int(m) for m in np.flatnonzero(md[:, 0] == METAL)], plain


def phi(world, rays, rng, w, max_depth, background=None):
    """sum_i <w_i, radiance_i> through radiance_rays (the products rounded, their sum exact), and the radiance."""
    L = art.radiance_rays(world, rays, rng=rng, spp=1, max_depth=max_depth, background=background)
    return math.fsum((w * L).ravel()), L


def grad_of(scene, kind, max_depth, **kw):
    rays, rng = paths_of(scene)
    return art.radiance_grad(world_of(scene), rays, weights_of(kind), rng=rng, spp=1, max_depth=max_depth, **kw)


def fd_bound(w, L, max_depth, h):
    """The rounding error allowed to a difference quotient of phi over 2h (the issue's bound): every path's radiance is a
    product of at most max_depth factors, each product within EPS; 4 covers the weights' product, the two evaluations and
    the gradient's own products.  4 * N_paths * max_depth * EPS * sum_i <|w_i|, |L_i|> / h."""
    return 4.0 * len(w) * max_depth * EPS * float((np.abs(w) * np.abs(L)).sum()) / h


# ------------------------------------------------------------------------------------------------ 1. the path is the renderer's
@pytest.mark.parametrize("scene", ["1", "2", "6", "7", "8", "cow", "9"])
def test_radiance_and_segments_are_radiance_rays(gpu, scene):
    rays, rng = paths_of(scene)
    want, st = art.radiance_rays(world_of(scene), rays, rng=rng, spp=1, stats=True)
    got, gt, gm, gb, gst = grad_of(scene, "positive", 50, stats=True)
    assert (bits(got) == bits(want)).all()
    assert gst["segments"] == st["segments"] and gst["primary"] == NP == st["primary"]
    assert want.max() > 0.0
    T, td = art.scene_textures(world_of(scene))
    M, md = art.scene_materials(world_of(scene))
    assert gt.shape == T.shape and gm.shape == M.shape and gb.shape == (3,)
    # only colour columns of solid textures and metal materials are written; everything else is +0.0
    assert (bits(gt[:, 3]) == 0).all() and (bits(gm[:, 3:]) == 0).all()
    assert (bits(gt[td[:, 0] != SOLID]) == 0).all() and (bits(gm[md[:, 0] != METAL]) == 0).all()
    assert np.isfinite(gt).all() and np.isfinite(gm).all() and np.isfinite(gb).all()
    assert np.abs(gt).max() + np.abs(gm).max() + np.abs(gb).max() > 0.0


def test_samples_per_ray_share_the_rays_weight(gpu):
    # spp samples of one ray with the weight w_i == spp rays with their own states and the weight repeated
    world, (rays, rng) = world_of("8"), paths_of("8")
    per_pixel = np.ascontiguousarray(rays[::SPP])  # one ray per pixel, 4 samples each, keyed by (seed, id, sample)
    w = np.array(weights_of("signed")[:W * H])
    L, gt, gm, gb = art.radiance_grad(world, per_pixel, w, spp=SPP, seed=5, id_base=7, max_depth=8)
    assert (bits(L) == bits(art.radiance_rays(world, per_pixel, spp=SPP, seed=5, id_base=7, max_depth=8))).all()
    parts = [art.radiance_grad(world, per_pixel, w, spp=1, seed=5, id_base=7, sample_base=s, max_depth=8) for s in range(SPP)]
    # the exact sums of the four calls' exact sums differ from the one call's only by the four roundings
    for whole, k in ((gt, 1), (gm, 2), (gb, 3)):
        total, size = sum(p[k] for p in parts), sum(np.abs(p[k]) for p in parts)
        assert (np.abs(whole - total) <= 8 * EPS * size).all()
    assert np.abs(gt).max() > 0.0


# ------------------------------------------------------------------------------------------------ 2. one product, exact
A, BG = (0.5, 0.25, 0.75), (1.0, 0.5, 0.25)


@functools.lru_cache(maxsize=None)
def one_sphere():
    art.reset_scene_rng()
    w = art.hittable_list()
    w.add(art.sphere((0.0, 0.0, 0.0), 1.0, art.lambertian(art.solid_color(*A))))
    return art.hittable_list(native=art.compile_world(w, 0))


def sphere_rays(towards):
    rnd = np.random.default_rng(5)
    n = 67  # a wave and three
    o = rnd.normal(size=(n, 3))
    o = 5.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    target = rnd.uniform(-0.5, 0.5, (n, 3))  # well inside the unit sphere
    d = target - o if towards else o - target
    return np.ascontiguousarray(np.concatenate([o, d, np.zeros((n, 1))], axis=1))


def test_one_lambertian_bounce_gives_the_products_exactly(gpu):
    world, rays = one_sphere(), sphere_rays(True)
    n, spp = len(rays), 8
    w = np.random.default_rng(6).integers(-16, 17, (n, 3)) / 8.0  # dyadic: every product and sum below is exact
    L, gt, gm, gb, st = art.radiance_grad(world, rays, w, spp=spp, max_depth=2, background=BG, seed=1, stats=True)
    assert st["segments"] == 2 * n * spp  # every path: the sphere, then the sky
    a, bg = np.array(A), np.array(BG)
    assert (bits(L) == bits(np.broadcast_to(spp * a * bg, (n, 3)))).all()
    assert gt.shape == (1, 4) and gm.shape == (1, 5)
    assert (bits(gt[0, :3]) == bits(spp * w.sum(0) * bg)).all() and (bits(gt[0, 3:]) == 0).all()
    assert (bits(gb) == bits(spp * w.sum(0) * a)).all()
    assert (bits(gm) == 0).all()


def test_rays_that_miss_everything_add_to_the_background_only(gpu):
    world, rays = one_sphere(), sphere_rays(False)
    n, spp = len(rays), 8
    w = np.random.default_rng(7).integers(-16, 17, (n, 3)) / 8.0
    L, gt, gm, gb = art.radiance_grad(world, rays, w, spp=spp, max_depth=2, background=BG)
    assert (bits(L) == bits(np.broadcast_to(spp * np.array(BG), (n, 3)))).all()
    assert (bits(gb) == bits(spp * w.sum(0))).all()
    assert (bits(gt) == 0).all() and (bits(gm) == 0).all()


# ------------------------------------------------------------------------------------------------ 3., 6. central differences
def directional_difference(scene, d_tex, d_mat, d_bg, h, max_depth, kind):
    """(phi(theta + h d) - phi(theta - h d)) / 2h through update_textures / update_materials + radiance_rays, and the
    rounding bound; the shared scene is put back as it was."""
    world, (rays, rng), w = world_of(scene), paths_of(scene), weights_of(kind)
    T0, _ = art.scene_textures(world)
    M0, _ = art.scene_materials(world)
    bg0 = np.array(world.background, np.float64)
    vals, bound = [], 0.0
    try:
        for sign in (1.0, -1.0):
            art.update_textures(world, T0 + sign * h * d_tex)
            art.update_materials(world, M0 + sign * h * d_mat)
            v, L = phi(world, rays, rng, w, max_depth, tuple(bg0 + sign * h * d_bg))
            vals.append(v)
            bound = max(bound, fd_bound(w, L, max_depth, h))
    finally:
        art.update_textures(world, T0)
        art.update_materials(world, M0)
    return (vals[0] - vals[1]) / (2.0 * h), bound


def direction(scene, which, rnd, lo=-1.0, hi=1.0):
    emit, att, metal, _ = structure(scene)
    T, _ = art.scene_textures(world_of(scene))
    M, _ = art.scene_materials(world_of(scene))
    d_tex, d_mat, d_bg = np.zeros_like(T), np.zeros_like(M), np.zeros(3)
    if which == "attenuation":
        d_tex[att, :3] = rnd.uniform(lo, hi, (len(att), 3))
        d_mat[metal, :3] = rnd.uniform(lo, hi, (len(metal), 3))
        assert len(att) + len(metal) > 0
    else:
        d_tex[emit, :3] = rnd.uniform(lo, hi, (len(emit), 3))
        d_bg[:] = rnd.uniform(lo, hi, 3)
    return d_tex, d_mat, d_bg


@pytest.mark.parametrize("scene,which", [("1", "attenuation"), ("2", "attenuation"), ("7", "attenuation"), ("8", "attenuation"),
                                         ("1", "emission"), ("6", "emission"), ("8", "emission")])
def test_central_differences_are_exact_at_depth_three(gpu, scene, which):
    """At max_depth 3 a path has at most two scatter vertices: phi has degree <= 2 in the attenuation colours and degree 1
    in the emitter colours and the background, so the central difference has no truncation error and differs from
    <grad, d> by rounding alone (fd_bound)."""
    h, depth = 2.0 ** -10, 3
    d_tex, d_mat, d_bg = direction(scene, which, np.random.default_rng(21))
    _, gt, gm, gb = grad_of(scene, "signed", depth)
    slope = float((gt * d_tex).sum() + (gm * d_mat).sum() + (gb * d_bg).sum())
    fd, bound = directional_difference(scene, d_tex, d_mat, d_bg, h, depth, "signed")
    print(f"scene {scene} {which}: <grad, d> {slope!r} central difference {fd!r} gap {abs(slope - fd):.3e} bound {bound:.3e}")
    assert bound < 1e-2 * abs(slope)  # the bound is far below the quantity it guards
    assert abs(slope - fd) <= bound
    assert slope != 0.0


def test_deep_paths_agree_with_central_differences(gpu):
    """Scene 6 at max_depth 50, where phi is a polynomial of high degree: the central differences at h = 2^-8 and 2^-9
    differ by delta, three quarters of the first one's truncation error (the error is c h^2 + O(h^4)), so the finer
    estimate lies within delta of the derivative up to O(h^4); 4 delta plus the rounding bound is allowed.  The direction
    raises every attenuation colour by 1/8 .. 1/4 and the weights are positive, so every term of the derivative is
    positive: it cannot be near zero, and with colours around 0.7 and paths of a dozen vertices the relative truncation
    error h^2 k^2 (d / c)^2 / 6 is of the order 1e-4 at h = 2^-8 -- below the 1e-3 the test demands of delta."""
    depth = 50
    d_tex, d_mat, d_bg = direction("6", "attenuation", np.random.default_rng(22), 0.125, 0.25)
    _, gt, gm, gb = grad_of("6", "positive", depth)
    slope = float((gt * d_tex).sum() + (gm * d_mat).sum() + (gb * d_bg).sum())
    (fd8, b8), (fd9, b9) = (directional_difference("6", d_tex, d_mat, d_bg, h, depth, "positive") for h in (2.0 ** -8, 2.0 ** -9))
    delta = abs(fd8 - fd9)
    print(f"<grad, d> {slope!r} central differences {fd8!r} {fd9!r} delta {delta:.3e} rounding bound {b9:.3e}")
    assert slope > 0.0
    assert delta < 1e-3 * abs(slope)
    assert abs(slope - fd9) <= 4.0 * delta + b9


# ------------------------------------------------------------------------------------------------ 4. order-free bits
def same_grads(a, b):
    return all((bits(x) == bits(y)).all() for x, y in zip(a[1:4], b[1:4]))


def test_the_same_call_twice_gives_the_same_bits(gpu):
    a, b = grad_of("8", "signed", 50), grad_of("8", "signed", 50)
    assert same_grads(a, b) and (bits(a[0]) == bits(b[0])).all()


def test_permuted_rays_give_the_same_bits(gpu):
    (rays, rng), w = paths_of("8"), weights_of("signed")
    perm = np.random.default_rng(31).permutation(NP)
    a = grad_of("8", "signed", 50)
    b = art.radiance_grad(world_of("8"), np.ascontiguousarray(rays[perm]), np.ascontiguousarray(w[perm]), rng=np.ascontiguousarray(rng[perm]),
                          spp=1, max_depth=50)
    assert same_grads(a, b) and (bits(a[0][perm]) == bits(b[0])).all()


def test_host_buffers_and_device_tensors_on_a_side_stream_agree(gpu):
    import torch
    (rays, rng), w = paths_of("8"), weights_of("signed")
    host = grad_of("8", "signed", 50)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_rays, d_w = torch.from_numpy(np.array(rays)).to("cuda"), torch.from_numpy(np.array(w)).to("cuda")
        d_rng = torch.from_numpy(np.array(rng).view(np.int64)).to("cuda")
        dev = art.radiance_grad(world_of("8"), d_rays, d_w, rng=d_rng, spp=1, max_depth=50)  # enqueued on `side`, not waited for
    assert all(x.is_cuda for x in dev)
    side.synchronize()
    assert same_grads(host, [x.cpu().numpy() for x in dev]) and (bits(dev[0].cpu().numpy()) == bits(host[0])).all()


def test_a_stream_that_is_not_torchs_current_one(gpu):
    # the inputs are complete before the call; the call runs on `side` while torch's current stream is its default one, on
    # which the wrapper must enqueue nothing that touches the outputs (they are made empty, and the call writes every cell)
    import torch
    (rays, rng), w = paths_of("8"), weights_of("signed")
    host = grad_of("8", "signed", 50)
    d_rays, d_w = torch.from_numpy(np.array(rays)).to("cuda"), torch.from_numpy(np.array(w)).to("cuda")
    d_rng = torch.from_numpy(np.array(rng).view(np.int64)).to("cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert torch.cuda.current_stream() != side
    dev = art.radiance_grad(world_of("8"), d_rays, d_w, rng=d_rng, spp=1, max_depth=50, stream=side)
    side.synchronize()
    assert same_grads(host, [x.cpu().numpy() for x in dev]) and (bits(dev[0].cpu().numpy()) == bits(host[0])).all()
    # the columns and rows no path adds to are written too: +0.0, not what the empty buffers held
    assert (bits(dev[1][:, 3].cpu().numpy()) == 0).all() and (bits(dev[2][:, 3:].cpu().numpy()) == 0).all()


def test_without_gradient_outputs_the_call_is_radiance_rays(gpu):
    # radiance alone through the C ABI (the wrapper always asks for gradients): nothing is recorded or walked back
    import ctypes
    from another_raytracer_amd._lib import lib, rt_radiance_params, rt_stats
    world, (rays, rng) = world_of("8"), paths_of("8")
    want, wst = art.radiance_rays(world, rays, rng=rng, spp=1, stats=True)
    q = rt_radiance_params(max_depth=50, spp=1)
    for c in range(3):
        q.background[c] = world.background[c]
    out, st, w = np.full((NP, 3), 7.0), rt_stats(), weights_of("signed")
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = lib.rt_radiance_grad(world.objects._native, ctypes.byref(q), ptr(rays), ptr(rng), ptr(w), NP, ptr(out), None, None, None, ctypes.byref(st))
    assert rc == 0 and (bits(out) == bits(want)).all() and st.segments == wst["segments"]
    # and a later call with gradients on the same scene is whole
    assert same_grads(grad_of("8", "signed", 50), grad_of("8", "signed", 50))


def test_the_global_scene_flag_changes_no_bit(gpu):
    a, b = grad_of("1", "signed", 50), grad_of("1", "signed", 50, global_scene=True)
    assert same_grads(a, b) and (bits(a[0]) == bits(b[0])).all()


# ------------------------------------------------------------------------------------------------ 5., 9. Euler's identity
def euler_sides(scene, world, L, w, gt, gb, background):
    """Radiance has degree 1 in the emitter colours and the background together: sum over emitter rows <G_t, c_t> +
    <G_bg, bg> = sum_i <w_i, radiance_i>."""
    emit, _, _, plain = structure(scene)
    assert plain
    T, _ = art.scene_textures(world)
    lhs = math.fsum((gt[emit, :3] * T[emit, :3]).ravel()) + math.fsum(gb * np.array(background))
    return lhs, math.fsum((w * L).ravel())


@pytest.mark.parametrize("scene", ["1", "6", "8"])
def test_eulers_identity_for_the_emitters(gpu, scene):
    depth = 50
    L, gt, gm, gb = grad_of(scene, "positive", depth)
    lhs, rhs = euler_sides(scene, world_of(scene), L, weights_of("positive"), gt, gb, world_of(scene).background)
    print(f"scene {scene}: emitters and background {lhs!r} radiance {rhs!r} gap {abs(lhs - rhs):.3e} bound {4.0 * NP * depth * EPS * rhs:.3e}")
    assert rhs > 0.0
    assert abs(lhs - rhs) <= 4.0 * NP * depth * EPS * rhs


def test_a_frame_larger_than_the_grid_on_device_tensors(gpu):
    # 256 x 144 x 8 = 294 912 paths against at most 196 608 lanes (256 CUs x 3 blocks x 256): lanes refill, and waves
    # claim new chunks while their other lanes walk back
    import torch
    w_, h_, k, depth = 256, 144, 8, 50
    world = world_of("1")
    # a persistent grid holds at most 3 blocks of 256 lanes per CU (three waves per SIMD): more paths than that
    assert w_ * h_ * k > torch.cuda.get_device_properties(0).multi_processor_count * 3 * 256
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rays, rng = art.camera_rays(camera_of(world, w_, h_), w_, h_, k, seed=SEED, device=0)
        w = torch.from_numpy(np.random.default_rng(41).uniform(0.25, 1.0, (w_ * h_ * k, 3))).to("cuda")
        L, gt, gm, gb, st = art.radiance_grad(world, rays, w, rng=rng, spp=1, max_depth=depth, stats=True)
        want, wst = art.radiance_rays(world, rays, rng=rng, spp=1, max_depth=depth, stats=True)
    side.synchronize()
    assert torch.equal(L.view(torch.int64), want.view(torch.int64)) and st["segments"] == wst["segments"]
    n = w_ * h_ * k
    lhs, rhs = euler_sides("1", world, L.cpu().numpy(), w.cpu().numpy(), gt.cpu().numpy(), gb.cpu().numpy(), world.background)
    print(f"emitters and background {lhs!r} radiance {rhs!r} gap {abs(lhs - rhs):.3e} bound {4.0 * n * depth * EPS * rhs:.3e}")
    assert rhs > 0.0 and abs(lhs - rhs) <= 4.0 * n * depth * EPS * rhs


# ------------------------------------------------------------------------------------------------ 7. after an update
def test_the_gradient_after_an_update_is_the_fresh_scenes(gpu, tmp_path):
    # scene 6 with new lamp colours through update_textures, against a scene made anew from those values: saved with
    # them and loaded as a new scene, whose upload derives the inlined colours on the host
    (rays, rng), w = paths_of("6"), weights_of("signed")
    world = art.scene_manager().build("6")  # its own copy: the update stays
    before = art.radiance_grad(world, rays, w, rng=rng, spp=1, max_depth=50)
    emit, _, _, plain = structure("6")
    T, _ = art.scene_textures(world)
    assert len(emit) > 0 and plain
    T[emit, :3] = T[emit, :3] * np.array([0.5, 1.25, 2.0]) + np.array([0.125, 0.0, 0.25])
    art.update_textures(world, T)
    updated = art.radiance_grad(world, rays, w, rng=rng, spp=1, max_depth=50)
    path = tmp_path / "lamps.art"
    art.save_scene(world, path)
    fresh_world = art.scene_manager().load(path)
    assert (bits(art.scene_textures(fresh_world)[0]) == bits(T)).all()
    fresh = art.radiance_grad(fresh_world, rays, w, rng=rng, spp=1, max_depth=50)
    assert same_grads(updated, fresh) and (bits(updated[0]) == bits(fresh[0])).all()
    assert not same_grads(updated, before)  # the attenuation rows carry the lamp's colour
    # the lamp's own row does not depend on its colour
    assert (bits(updated[1][emit]) == bits(before[1][emit])).all()


# ------------------------------------------------------------------------------------------------ 8. the Python layers
@pytest.mark.parametrize("place", ["numpy", "cuda"])
def test_render_grad_is_radiance_grad_of_the_camera_rays(gpu, place):
    world = world_of("8")
    cam = camera_of(world, W, H)
    adj = np.random.default_rng(51).uniform(-1.0, 1.0, (H, W, 3))
    if place == "numpy":
        acc, gt, gm, gb = art.render_grad(world, cam, W, H, SPP, adj, seed=SEED)
    else:  # a tensor adjoint: everything runs on torch's current stream, here a side stream
        import torch
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            out = art.render_grad(world, cam, W, H, SPP, torch.from_numpy(adj).to("cuda"), seed=SEED)
        assert all(x.is_cuda for x in out)
        side.synchronize()
        acc, gt, gm, gb = (x.cpu().numpy() for x in out)
    rays, rng = paths_of("8")
    L, wt, wm, wb = art.radiance_grad(world, rays, np.ascontiguousarray(np.repeat(adj.reshape(-1, 3), SPP, axis=0)), rng=rng, spp=1)
    assert same_grads((None, gt, gm, gb), (None, wt, wm, wb))
    eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=SPP, seed=SEED)
    eng.set_scene(world.objects, world.background)
    img, want = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3))
    eng.run(img, accum=want)
    assert acc.shape == (H, W, 3) and (bits(acc) == bits(want)).all()


@pytest.mark.parametrize("place", ["cpu", "cuda"])
def test_the_autograd_function_hands_back_the_direct_calls_rows(gpu, place):
    import torch
    world = art.scene_manager().build("8")  # its own copy: the forward pass writes the parameters into the scene
    (rays, rng), w = paths_of("8"), weights_of("signed")
    T0, _ = art.scene_textures(world)
    M0, _ = art.scene_materials(world)
    bg0 = np.array(world.background, np.float64) + 0.125
    t_rays, t_w = torch.from_numpy(np.array(rays)).to(place), torch.from_numpy(np.array(w)).to(place)
    t_rng = torch.from_numpy(np.array(rng).view(np.int64)).to(place) if place == "cuda" else np.array(rng)
    tex = torch.from_numpy(T0).to(place).requires_grad_()
    mat = torch.from_numpy(M0).to(place).requires_grad_()
    bg = torch.from_numpy(bg0).to(place).requires_grad_()
    L = art.differentiable_radiance(world, t_rays, tex, mat, bg, rng=t_rng, max_depth=12)
    assert L.requires_grad and tuple(L.shape) == (NP, 3)
    (L * t_w).sum().backward()
    want = art.radiance_grad(world, rays, w, rng=rng, spp=1, max_depth=12, background=tuple(bg0))
    assert (bits(L.detach().cpu().numpy()) == bits(want[0])).all()
    assert same_grads(want, (None, tex.grad.cpu().numpy(), mat.grad.cpu().numpy(), bg.grad.cpu().numpy()))
    assert tex.grad.device == tex.device and np.abs(want[3]).max() > 0.0
    # a parameter that was not given gets no gradient, and the others are the same
    tex.grad = None
    L = art.differentiable_radiance(world, t_rays, tex, None, None, rng=t_rng, max_depth=12, )
    (L * t_w).sum().backward()
    want = art.radiance_grad(world, rays, w, rng=rng, spp=1, max_depth=12)
    assert (bits(tex.grad.cpu().numpy()) == bits(want[1])).all()


def test_zero_weights_give_zero_arrays(gpu):
    rays, rng = paths_of("8")
    L, gt, gm, gb = art.radiance_grad(world_of("8"), rays, np.zeros((NP, 3)), rng=rng, spp=1)
    assert (bits(gt) == 0).all() and (bits(gm) == 0).all() and (bits(gb) == 0).all()
    assert L.max() > 0.0


def test_a_refused_workspace_fails_the_call_and_the_next_one_works(gpu, options):
    # an injected allocation refusal on the host (test.fault_workspace_bytes), on a scene of its own: its workspace is empty
    world = art.scene_manager().build("c1")
    rays, _ = art.camera_rays(camera_of(world, W, H), W, H, 1, seed=1)
    w = np.array(weights_of("signed")[:len(rays)])
    want = art.radiance_grad(world_of("c1"), rays, w, spp=SPP, seed=4)
    options("test.fault_workspace_bytes", 4096)
    with pytest.raises(art.RTError, match="RT_E_DEVICE"):
        art.radiance_grad(world, rays, w, spp=SPP, seed=4)
    options("test.fault_workspace_bytes", 0)
    got = art.radiance_grad(world, rays, w, spp=SPP, seed=4)
    assert same_grads(want, got) and (bits(want[0]) == bits(got[0])).all()
