"""Colour gradients of path-traced radiance (rt_radiance_grad, include/art.h): the exact derivative of radiance_rays'
radiance with respect to every solid texture colour, every metal albedo and the background, in one call whatever the
number of colours (measured: 1.4 to 4.3 radiance_rays calls) -- the derivative an optimiser that drives
update_textures / update_materials needs, without one render per parameter.

    rays, rng = art.camera_rays(cam, W, H, spp)
    L, gT, gM, gB = art.radiance_grad(world, rays, weights, rng=rng)      # weights: (n, 3) = d loss / d L
    T, _ = art.scene_textures(world)
    art.update_textures(world, T - lr * gT)                                # a descent step

    acc, gT, gM, gB = art.render_grad(world, cam, W, H, spp, image_adjoint)   # the adjoint of engine.run's accum
    L = art.differentiable_radiance(world, rays, textures, materials)         # a torch.autograd.Function; L.backward()

gT is (T, 4) and gM (M, 5) in scene_textures' / scene_materials' row layout: only the colour columns of solid textures
and metal materials are non-zero.  The sums are exact (wide integers, rounded once), so the gradient's bits depend on
neither the order of the rays nor the device.

Image textures (rt_radiance_grad_texels): texels=True returns one more array, (N, 3), a row per texel of the scene's
images in scene_images' global order -- the derivative with respect to the texel's value, byte / 255 per channel:

    desc, first, _ = art.scene_images(world)
    L, gT, gM, gB, gX = art.radiance_grad(world, rays, weights, rng=rng, texels=True)
    w, h, _ = desc[0]
    g_earth = gX[first[0]:first[0] + w * h].reshape(h, w, 3)              # the gradient of image 0, as scene_texels lays it out
"""
import ctypes

import numpy as np

from ._buffers import address, same_place, scene_background, stream_handle
from ._lib import RT_GLOBAL_SCENE, RT_OUT_DEVICE, check, lib, rt_radiance_params, rt_stats
from .appearance import MATERIAL_DOUBLES, TEXTURE_DOUBLES, scene_images, scene_texels, update_materials, update_texels, update_textures
from .rays import _native_scene, _rays, camera_rays, radiance_rays


def radiance_grad(objects, rays, weights, spp=1, max_depth=50, seed=0, sample_base=0, id_base=0, rng=None, background=None,
                  global_scene=False, out_radiance=None, stream=None, stats=False, texels=False):
    """rt_radiance_grad over a compiled scene: radiance_rays' paths (rays, spp, max_depth, seed, sample_base, id_base, rng,
    background, global_scene, stream as there) and the gradient of sum_i <weights[i], radiance[i]>.

    weights: (n, 3) float64, the adjoint of radiance[i]; it applies to each of ray i's spp paths.  Returns (radiance (n, 3),
    grad_textures (T, 4), grad_materials (M, 5), grad_background (3,)); with stats=True a dict with segments, primary and
    ms follows.  radiance (`out_radiance`, or a new buffer) holds radiance_rays' bits.  Buffers are numpy arrays (the call
    copies and blocks) or contiguous tensors on the scene's device, used in place on `stream`; the results are of the kind
    the rays are.  Calls on one scene share its workspace: order them on one stream, or synchronise between them.

    texels=True (rt_radiance_grad_texels): grad_texels (N, 3) follows grad_background -- a row per texel of the scene's
    images, global texel first_texel[k] + j * w + i of scene_images; the other results keep their bits."""
    handle = _native_scene(objects)
    n, rays_ptr, dev = _rays(rays, handle.device)
    spp = int(spp)
    if spp < 1:
        raise ValueError("spp must be >= 1")
    if not hasattr(weights, "shape"):
        raise TypeError("weights must be a numpy array or a torch tensor")
    w_ptr, w_dev = address(weights, "weights", ("float64",), shape=(n, 3), device_index=handle.device)
    rng_ptr, rng_dev = (None, None) if rng is None else address(rng, "rng", ("uint64",), shape=(n * spp,), device_index=handle.device,
                                                                tensor_dtypes=("int64", "uint64"))
    n_tex = check(lib.rt_scene_textures_get(handle, None, None, 0), "scene_textures")
    n_mat = check(lib.rt_scene_materials_get(handle, None, None, 0), "scene_materials")
    # The call writes every element of every output, so the buffers are made empty: on a device nothing is enqueued on
    # torch's current stream, which `stream` need not be.  (No rays: the call writes nothing, and the gradient is zero.)
    if dev:
        import torch

        def new(*shape):
            return (torch.empty if n else torch.zeros)(shape, dtype=torch.float64, device=rays.device)
    else:
        def new(*shape):
            return (np.empty if n else np.zeros)(shape, np.float64)
    if out_radiance is None:
        out_radiance = new(n, 3)
    out_ptr, out_dev = address(out_radiance, "out_radiance", ("float64",), shape=(n, 3), device_index=handle.device)
    same_place(rays=dev, weights=w_dev, rng=rng_dev, out_radiance=out_dev)
    g_tex, g_mat, g_bg = new(n_tex, TEXTURE_DOUBLES), new(n_mat, MATERIAL_DOUBLES), new(3)
    g_tx = None
    if texels:
        desc, _, _ = scene_images(objects)
        g_tx = new(int((desc[:, 0].astype(np.int64) * desc[:, 1]).sum()), 3)
    background = scene_background(objects, handle, background)
    q = rt_radiance_params()
    q.flags = (RT_OUT_DEVICE if dev else 0) | (RT_GLOBAL_SCENE if global_scene else 0)
    q.spp, q.max_depth, q.sample_base, q.seed, q.id_base = spp, int(max_depth), int(sample_base), int(seed), int(id_base)
    for c in range(3):
        q.background[c] = float(background[c])
    q.stream = stream_handle(stream, rays.device if dev else None)
    st = rt_stats()

    def ptr(a):
        return ctypes.c_void_p(a.data_ptr() if dev else a.ctypes.data)
    head = (handle, ctypes.byref(q), ctypes.c_void_p(rays_ptr), None if rng_ptr is None else ctypes.c_void_p(rng_ptr), ctypes.c_void_p(w_ptr), n,
            ctypes.c_void_p(out_ptr), ptr(g_tex), ptr(g_mat), ptr(g_bg))
    if texels:
        check(lib.rt_radiance_grad_texels(*head, ptr(g_tx), ctypes.byref(st) if stats else None), "radiance_grad")
    else:
        check(lib.rt_radiance_grad(*head, ctypes.byref(st) if stats else None), "radiance_grad")
    res = (out_radiance, g_tex, g_mat, g_bg) + ((g_tx,) if texels else ())
    return res + ({"segments": st.segments, "primary": st.primary, "ms": st.ms},) if stats else res


def render_grad(objects, cam, width, height, spp, image_adjoint, seed=0, max_depth=50, background=None, global_scene=False, texels=False):
    """The gradient of a whole frame: camera_rays(cam, width, height, spp, seed), then radiance_grad on those rays and
    states, one path per ray.  image_adjoint: (height, width, 3) float64, the adjoint of engine.run's accum (the per-pixel
    sums over the samples); it applies to every sample of its pixel.  A numpy array, or a tensor on the scene's device:
    the rays are then made there, and everything -- the library's calls and the torch operations that repeat the adjoint
    and sum the samples -- runs on torch's current stream (make a side stream current to use it).  Returns (accum
    (height, width, 3): the in-order sums engine.run gives, grad_textures, grad_materials, grad_background), and with
    texels=True radiance_grad's grad_texels (N, 3) after them."""
    if not hasattr(image_adjoint, "shape"):
        raise TypeError("image_adjoint must be a numpy array or a torch tensor")
    width, height, spp = int(width), int(height), int(spp)
    if tuple(image_adjoint.shape) != (height, width, 3):
        raise ValueError("image_adjoint must have shape (height, width, 3)")
    tensor = not isinstance(image_adjoint, np.ndarray)
    rays, rng = camera_rays(cam, width, height, spp, seed=seed, device=image_adjoint.device if tensor else None)
    if tensor:
        weights = image_adjoint.reshape(height * width, 1, 3).expand(-1, spp, -1).reshape(-1, 3).contiguous()
    else:
        weights = np.ascontiguousarray(np.repeat(image_adjoint.reshape(height * width, 3), spp, axis=0))
    L, *grads = radiance_grad(objects, rays, weights, spp=1, max_depth=max_depth, rng=rng, background=background, global_scene=global_scene,
                              texels=texels)
    L = L.reshape(height, width, spp, 3)
    acc = 0.0 + L[:, :, 0]
    for s in range(1, spp):  # in sample order from +0.0, as k_accum
        acc = acc + L[:, :, s]
    return (acc, *grads)


_function = None


def _autograd_function():
    """The torch.autograd.Function behind differentiable_radiance, made at the first call (torch is imported lazily)."""
    global _function
    if _function is not None:
        return _function
    import torch

    def buf(t):  # the package's buffer for a tensor: a device tensor as it is, a CPU tensor as a numpy array
        t = t.detach().contiguous()
        return t if t.is_cuda else t.numpy()

    class RadianceFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, textures, materials, background, rays, world, kw, images, *texels):
            # texels[k]: (h, w, 3) values in [0, 1] for image images[k]: the bytes clamp(round(255 x)) go into the image's
            # first three channels, a fourth byte stays
            for image, x in zip(images, texels):
                new = torch.clamp(torch.round(x.detach().to(torch.float64) * 255.0), 0.0, 255.0).to(torch.uint8)
                if x.is_cuda:
                    now = torch.from_numpy(scene_texels(world, image)).to(x.device)
                    now[:, :, :3] = new
                    update_texels(world, image, now.contiguous())
                else:
                    now = scene_texels(world, image)
                    now[:, :, :3] = new.numpy()
                    update_texels(world, image, now)
            ctx.images, ctx.texel_like = tuple(images), [(x.device, x.dtype, tuple(x.shape)) for x in texels]
            if textures is not None:
                update_textures(world, buf(textures))
            if materials is not None:
                update_materials(world, buf(materials))
            ctx.world, ctx.kw = world, dict(kw)
            ctx.kw["background"] = None if background is None else tuple(float(x) for x in background.detach().cpu().tolist())
            ctx.rays = rays.detach().contiguous()
            ctx.like = [None if t is None else (t.device, t.dtype) for t in (textures, materials, background)]
            out = radiance_rays(world, buf(ctx.rays), **ctx.kw)
            return out if hasattr(out, "data_ptr") else torch.from_numpy(out)

        @staticmethod
        def backward(ctx, grad_out):
            w = grad_out.detach().to(torch.float64).contiguous()
            _, g_tex, g_mat, g_bg, *g_tx = radiance_grad(ctx.world, buf(ctx.rays), buf(w), texels=bool(ctx.images), **ctx.kw)
            grads = []
            for g, like in zip((g_tex, g_mat, g_bg), ctx.like):
                if like is None:
                    grads.append(None)
                else:
                    g = g if hasattr(g, "data_ptr") else torch.from_numpy(g)
                    grads.append(g.to(device=like[0], dtype=like[1]))
            texel_grads = []
            if ctx.images:  # straight-through: the value is byte / 255, and the gradient that of the value
                desc, first, _ = scene_images(ctx.world)
                g = g_tx[0] if hasattr(g_tx[0], "data_ptr") else torch.from_numpy(g_tx[0])
                for image, (device, dtype, shape) in zip(ctx.images, ctx.texel_like):
                    wd, ht = int(desc[image, 0]), int(desc[image, 1])
                    rows = g[int(first[image]):int(first[image]) + wd * ht].reshape(ht, wd, 3)
                    texel_grads.append(rows.to(device=device, dtype=dtype))
            return (*grads, None, None, None, None, *texel_grads)

    _function = RadianceFunction
    return _function


def differentiable_radiance(objects, rays, textures=None, materials=None, background=None, spp=1, max_depth=50, seed=0, sample_base=0, id_base=0,
                            rng=None, global_scene=False, texels=None):
    """radiance_rays as a differentiable torch operation.  textures ((T, 4), scene_textures' rows), materials ((M, 5),
    scene_materials' rows) and background ((3,)) are float64 tensors, any of them None: the forward pass writes the given
    ones into the scene (update_textures / update_materials) and returns radiance_rays' (n, 3) tensor; backward() calls
    radiance_grad with the incoming adjoint and hands each given tensor its gradient.  rays ((n, 7)) and the parameters
    live on the scene's device (used in place, on torch's current stream) or on the CPU.  The scene keeps the values of
    the last forward pass.

    texels: {image: tensor (h, w, 3)}, float values in [0, 1] for the first three channels of the scene's image `image`
    (scene_images' index; an image with bpp >= 3).  The forward pass writes the bytes clamp(round(255 x)) (update_texels;
    a fourth byte of the image stays), so it is piecewise constant in x: a change of x below half a byte step renders
    the same image.  backward() hands each tensor that image's rows of radiance_grad's texel gradient, reshaped (h, w, 3):
    the derivative with respect to the value byte / 255 the renderer used, passed straight through the rounding."""
    fn = _autograd_function()
    kw = dict(spp=spp, max_depth=max_depth, seed=seed, sample_base=sample_base, id_base=id_base, rng=rng, global_scene=global_scene)
    images = tuple(int(k) for k in (texels or {}))
    if images:
        desc, _, _ = scene_images(objects)
        for k in images:
            if not 0 <= k < len(desc):
                raise IndexError(f"image {k} is not one of the scene's {len(desc)} images")
            want = (int(desc[k, 1]), int(desc[k, 0]), 3)
            if int(desc[k, 2]) < 3 or not hasattr(texels[k], "data_ptr") or tuple(texels[k].shape) != want or not texels[k].is_floating_point():
                raise ValueError(f"texels[{k}] must be a float tensor of shape {want} for an image with at least three bytes per texel")
    return fn.apply(textures, materials, background, rays, objects, kw, images, *(texels[k] for k in images))
