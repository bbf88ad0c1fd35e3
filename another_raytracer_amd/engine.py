"""engine / camera surface of the reference (src/engine/engine.h, src/engine/camera.h), on libart.so.

`engine.run(out)` is the drop-in for engine<W,H,C>::run (engine.h:30-54): it renders every pixel with the
reference's sampling (`_stochastic_sample`, engine.h:58-68) and integrator (`_ray_color`, engine.h:447-466) on the
GPU and writes write_color's RGB8 (color.h:6-22) into `out`.  The reference's compile-time tracer_constants
(tracer_constants.h:6-14) are constructor arguments here.
"""
import ctypes
import enum

import numpy as np

from ._lib import RT_ADAPTIVE, RT_DN_NO_DEMODULATE, RT_FP64, RT_GUIDE_DOUBLES, rt_denoise_params, RT_PARALLEL_IMAGES, rt_progress_fn, RT_GLOBAL_SCENE, RT_OUT_DEVICE, RT_PROFILE, RT_SPLIT_SHADE, RT_WAVEFRONT, check, dvec, lib, rt_camera, rt_params, rt_stats
from ._buffers import ANY, address, same_place
from .scene import compile_world


class tracer_constants:  # tracer_constants.h:6-14
    aspect_ratio = 4.0 / 3.0
    image_width = 720
    image_height = int(image_width / aspect_ratio)
    color_channels = 3
    samples_per_pixel = 100
    max_depth = 50


class engine_mode(enum.Enum):  # engine.h:10-16
    single = 0
    adaptive = 1
    parallel_stripes = 2
    parallel_images = 3


class camera:  # camera.h:8-36
    def __init__(self, lookfrom, lookat, vup, vfov, aspect_ratio, aperture, focus_dist, time0=0.0, time1=0.0):
        self.c = rt_camera(dvec(lookfrom), dvec(lookat), dvec(vup), float(vfov), float(aspect_ratio), float(aperture),
                           float(focus_dist), float(time0), float(time1))


def _pointer(out, nbytes, what="output"):
    """(address, is_device) of a frame of RGB8 bytes: a uint8 numpy array, or a tensor (CPU or device) of >= nbytes bytes."""
    return address(out, what, ("uint8",), min_bytes=nbytes, tensor_dtypes=ANY)


def _f64(buf, what, count):
    """(address, is_device) of >= count float64 elements: a numpy array, or a tensor (CPU or device) of 8-byte elements."""
    return address(buf, what, ("float64",), at_least=count, tensor_dtypes=8)


def _denoise_params(width, height, iterations=0, normal_squarings=0, sigma_color=0.0, sigma_plane=0.0, albedo_floor=0.0,
                    demodulate=True, stream=None):
    """rt_denoise_params; 0 keeps a field's default (include/art.h: 5 iterations, 6 squarings, sigma_color 1,
    sigma_plane 0.1, albedo_floor 0.5)."""
    d = rt_denoise_params()
    d.width, d.height = int(width), int(height)
    d.iterations, d.normal_squarings = int(iterations), int(normal_squarings)
    d.sigma_color, d.sigma_plane, d.albedo_floor = float(sigma_color), float(sigma_plane), float(albedo_floor)
    d.flags = 0 if demodulate else RT_DN_NO_DEMODULATE
    d.stream = stream
    return d


def denoise(accum_a, accum_b, spp_each, guides, out_color=None, out_rgb8=None, device=0, **denoise_options):
    """rt_denoise: the variance-guided a-trous filter over two half-renders (H x W x 3 float64 radiance sums of
    spp_each samples each, rendered with different seeds) and the frame's guides (engine.render_guides, H x W x 10).
    Returns (out_color, ms): the filtered per-sample radiance (H x W x 3 float64; allocated next to accum_a unless
    given) and the device time of the filter.  out_rgb8 (optional, uint8 H x W x 3) receives write_color of it.  All
    buffers live on the host (numpy) or all on `device` (torch).  denoise_options: iterations, normal_squarings,
    sigma_color, sigma_plane, albedo_floor, demodulate, stream."""
    if accum_a.ndim != 3 or accum_a.shape[2] != 3:
        raise ValueError("accum_a must have shape (H, W, 3)")
    h, w = int(accum_a.shape[0]), int(accum_a.shape[1])
    n = h * w
    if out_color is None:
        if isinstance(accum_a, np.ndarray):
            out_color = np.empty((h, w, 3), np.float64)
        else:
            import torch
            out_color = torch.empty((h, w, 3), dtype=torch.float64, device=accum_a.device)
    bufs = {"accum_a": (accum_a, 3 * n), "accum_b": (accum_b, 3 * n), "guides": (guides, RT_GUIDE_DOUBLES * n), "out_color": (out_color, 3 * n)}
    ptrs, where = zip(*(_f64(buf, what, count) for what, (buf, count) in bufs.items()))
    rgb_ptr, rgb_dev = (None, None) if out_rgb8 is None else _pointer(out_rgb8, 3 * n, "out_rgb8")
    dev = same_place(**dict(zip(bufs, where)), out_rgb8=rgb_dev)
    p = _denoise_params(w, h, **denoise_options)
    if dev:
        p.flags |= RT_OUT_DEVICE
    ms = ctypes.c_double()
    check(lib.rt_denoise(int(device), ctypes.byref(p), ctypes.c_void_p(ptrs[0]), ctypes.c_void_p(ptrs[1]), int(spp_each),
                         ctypes.c_void_p(ptrs[2]), ctypes.c_void_p(ptrs[3]), ctypes.c_void_p(rgb_ptr) if rgb_ptr else None,
                         ctypes.byref(ms)), "denoise")
    return out_color, ms.value


class engine:
    """engine<W,H,C>(const camera&, engine_mode) (engine.h:19-476)."""

    def __init__(self, cam, mode=engine_mode.single, width=tracer_constants.image_width,
                 height=tracer_constants.image_height, samples_per_pixel=tracer_constants.samples_per_pixel,
                 max_depth=tracer_constants.max_depth, device=0, seed=0, precision="f64", samples_per_pass=0):
        self.cam, self.m = cam, mode
        self.width, self.height = int(width), int(height)
        self.samples_per_pixel, self.max_depth = int(samples_per_pixel), int(max_depth)
        self.device, self.seed = int(device), int(seed)
        if precision != "f64":
            raise ValueError("precision must be 'f64': the reference's double arithmetic is the only mode (ABI 2)")
        self.precision = precision
        self.samples_per_pass = int(samples_per_pass)
        # True forces the global-memory extend kernel even when the scene fits the LDS-resident variant (A/B, tests)
        self.global_scene = False
        # True keeps shading in separate per-material k_shade launches even when it could be fused (A/B, tests)
        self.split_shade = False
        # True runs the fused LDS kernel once per bounce depth instead of the persistent-path kernel (A/B, tests)
        self.wavefront = False
        self.world = None
        self.background = (0.0, 0.0, 0.0)
        self._scene = None
        self.stats = {}

    def set_scene(self, world, background):  # engine.h:24-28
        self.world = world
        self.background = tuple(float(x) for x in background)
        self._scene = None if world is None or world.empty() else compile_world(world, self.device)

    def scene_info(self):
        """rt_scene_info of the engine's compiled scene (device_bytes_f64 is set once a render uploaded it)."""
        from ._lib import rt_scene_info
        if self._scene is None:
            raise ValueError("no scene set")
        info = rt_scene_info()
        check(lib.rt_scene_info_get(self._scene, ctypes.byref(info)), "rt_scene_info_get")
        return {f: (tuple(getattr(info, f)) if isinstance(getattr(info, f), ctypes.Array) else getattr(info, f)) for f, _ in info._fields_}

    def params(self, band_rows=None, band_count=1, band_index=0, flags=0, stream=None):
        p = rt_params()
        p.width, p.height = self.width, self.height
        p.spp, p.max_depth, p.seed = self.samples_per_pixel, self.max_depth, self.seed
        p.fp_mode = RT_FP64
        p.band_rows = band_rows or self.height
        p.band_count, p.band_index = band_count, band_index
        p.samples_per_pass, p.flags = self.samples_per_pass, flags
        p.stream = stream
        for c in range(3):
            p.background[c] = self.background[c]
        return p

    def run(self, output_image, accum=None, band_rows=None, band_count=1, band_index=0, profile=False, stream=None):
        """Renders into output_image (uint8, local_rows x W x 3).  Returns elapsed ms, or -1 on an empty world
        (engine.h:32-36).  `accum` (optional, float64 local_rows x W x 3) receives the per-pixel radiance sums.
        engine_mode.adaptive runs _run_adaptive (engine.h:151-333) on the GPU; engine_mode.parallel_images runs
        _run_parallel_images (engine.h:378-445: four float partial images of spp/4 samples, summed); single and
        parallel_stripes compute the same image (their only difference is the reference's CPU threading)."""
        if self._scene is None:
            print("Invalid input scene!")
            return -1
        adaptive = self.m == engine_mode.adaptive
        if adaptive and (self.width % 12 or self.height % 12):
            # engine.h:178-179
            raise ValueError("for adaptive strategy image size should perfectly fit big square size for now!!")
        if adaptive and accum is not None:
            raise ValueError("engine_mode.adaptive interpolates most pixels: there are no radiance sums to return")
        flags = ((RT_PROFILE if profile else 0) | (RT_GLOBAL_SCENE if self.global_scene else 0)
                 | (RT_SPLIT_SHADE if self.split_shade else 0) | (RT_ADAPTIVE if adaptive else 0)
                 | (RT_PARALLEL_IMAGES if self.m == engine_mode.parallel_images else 0)
                 | (RT_WAVEFRONT if self.wavefront else 0))
        p = self.params(band_rows, band_count, band_index, flags, stream)
        rows = check(lib.rt_local_rows(ctypes.byref(p), None), "rt_local_rows")
        nbytes = rows * self.width * 3
        ptr, dev = _pointer(output_image, nbytes, "output_image")
        acc_ptr, acc_dev = (None, None) if accum is None else address(accum, "accum", ANY, min_bytes=nbytes * 8)
        if same_place(output_image=dev, accum=acc_dev):
            p.flags |= RT_OUT_DEVICE
        st = rt_stats()
        check(lib.rt_render(self._scene, ctypes.byref(self.cam.c), ctypes.byref(p), ctypes.c_void_p(ptr),
                            ctypes.c_void_p(acc_ptr) if acc_ptr else None, ctypes.byref(st)), "engine.run")
        self.stats = st.as_dict()
        return int(round(st.ms))

    def tile_candidates(self, band_rows=None, band_count=1, band_index=0):
        """rt_tile_candidates: the per-tile sphere lists run() would build (option render.tile_lists: 0 off, 1 when a
        pass holds at least 72 samples per pixel, 2 always), as a uint16 array (tile rows, tile columns) of candidate
        counts, 0xFFFF for a tile with more than 15 spheres, whose batches walk the tree; None when run() builds no
        lists (the scene, the option, the mode or the sample count)."""
        if self._scene is None:
            raise ValueError("no scene set")
        flags = ((RT_GLOBAL_SCENE if self.global_scene else 0) | (RT_SPLIT_SHADE if self.split_shade else 0)
                 | (RT_ADAPTIVE if self.m == engine_mode.adaptive else 0)
                 | (RT_PARALLEL_IMAGES if self.m == engine_mode.parallel_images else 0) | (RT_WAVEFRONT if self.wavefront else 0))
        p = self.params(band_rows, band_count, band_index, flags)
        rows = check(lib.rt_local_rows(ctypes.byref(p), None), "rt_local_rows")
        tx, ty = (self.width + 7) // 8, (rows + 7) // 8
        counts = np.zeros((ty, tx), np.uint16)
        n = check(lib.rt_tile_candidates(self._scene, ctypes.byref(self.cam.c), ctypes.byref(p), ctypes.c_void_p(counts.ctypes.data), tx * ty),
                  "engine.tile_candidates")
        return counts if n else None

    def render_guides(self, guides=None, rays=None, band_rows=None, band_count=1, band_index=0, stream=None):
        """First-hit guide buffers (rt_render_guides): float64 (local_rows, W, 10) = albedo, normal, position, t of the
        pixel-centre ray of every local pixel (a miss: t = position = inf, normal 0, albedo 1).  `guides` / `rays`
        (optional, (local_rows, W, 7): the rays themselves, as rt_trace_rays takes them) may be numpy arrays or
        device tensors; returns the guides array."""
        if self._scene is None:
            raise ValueError("no scene set")
        p = self.params(band_rows, band_count, band_index, RT_GLOBAL_SCENE if self.global_scene else 0, stream)
        rows = check(lib.rt_local_rows(ctypes.byref(p), None), "rt_local_rows")
        n = rows * self.width
        if guides is None:
            guides = np.empty((rows, self.width, RT_GUIDE_DOUBLES), np.float64)
        ptr, dev = _f64(guides, "guides", RT_GUIDE_DOUBLES * n)
        rays_ptr, rays_dev = (None, None) if rays is None else _f64(rays, "rays", 7 * n)
        if same_place(guides=dev, rays=rays_dev):
            p.flags |= RT_OUT_DEVICE
        check(lib.rt_render_guides(self._scene, ctypes.byref(self.cam.c), ctypes.byref(p), ctypes.c_void_p(ptr),
                                   ctypes.c_void_p(rays_ptr) if rays_ptr else None), "engine.render_guides")
        return guides

    def run_denoised(self, output_image, color=None, **denoise_options):
        """One-call denoised render (rt_render_denoised): two half-renders of samples_per_pixel / 2 samples (seeds
        `seed` and `seed + 1`), the guide pass and the a-trous filter, all on the device; output_image (uint8 H x W x
        3) receives write_color of the filtered frame and `color` (optional float64 H x W x 3) the frame itself.
        samples_per_pixel must be even.  denoise_options as for denoise().  Returns elapsed ms (the whole call), or -1
        on an empty world."""
        if self._scene is None:
            print("Invalid input scene!")
            return -1
        if self.m in (engine_mode.adaptive, engine_mode.parallel_images):
            raise ValueError("run_denoised renders whole frames of independent samples (engine_mode.adaptive / parallel_images do not)")
        flags = ((RT_GLOBAL_SCENE if self.global_scene else 0) | (RT_SPLIT_SHADE if self.split_shade else 0)
                 | (RT_WAVEFRONT if self.wavefront else 0))
        p = self.params(None, 1, 0, flags, denoise_options.pop("stream", None))
        n = self.height * self.width
        ptr, dev = _pointer(output_image, 3 * n, "output_image")
        color_ptr, color_dev = (None, None) if color is None else _f64(color, "color", 3 * n)
        if same_place(output_image=dev, color=color_dev):
            p.flags |= RT_OUT_DEVICE
        d = _denoise_params(self.width, self.height, **denoise_options)
        st = rt_stats()
        check(lib.rt_render_denoised(self._scene, ctypes.byref(self.cam.c), ctypes.byref(p), ctypes.byref(d), ctypes.c_void_p(ptr),
                                     ctypes.c_void_p(color_ptr) if color_ptr else None, ctypes.byref(st)), "engine.run_denoised")
        self.stats = st.as_dict()
        return int(round(st.ms))

    def run_noise_target(self, output_image, accum=None, counts=None, moments=None, **noise_options):
        """Noise-target render (rt_render_noise_target): every pixel is traced until the standard error of its mean
        luminance is within rel_tol of the mean (+ lum_floor), up to samples_per_pixel samples (the per-pixel cap).
        output_image (uint8, local_rows x W x 3) receives write_color of every pixel's sums with its own count;
        optional: accum (float64 rows x W x 3 radiance sums), counts (int32 rows x W samples per pixel), moments
        (float64 rows x W x 2: the luminance sums S1, S2).  numpy arrays, or torch tensors all on the device.
        noise_options: min_spp, step_spp, dilate, rel_tol, lum_floor (0 / omitted = the defaults 32, 32, 0, 0.05, 0.01),
        and band_rows, band_count, band_index, profile, stream as for run().  A pixel with n samples equals run() at
        samples_per_pixel = n bit for bit.  Returns {"rounds", "converged_pixels", "samples", "ms"}, or None on an
        empty world."""
        from ._lib import rt_noise_params, rt_noise_result
        if self._scene is None:
            print("Invalid input scene!")
            return None
        if self.m in (engine_mode.adaptive, engine_mode.parallel_images) or self.split_shade or self.wavefront:
            raise ValueError("run_noise_target traces engine_mode.single samples through the persistent-path kernels "
                             "(no adaptive / parallel_images mode, split_shade or wavefront)")
        opts = dict(noise_options)
        flags = (RT_PROFILE if opts.pop("profile", False) else 0) | (RT_GLOBAL_SCENE if self.global_scene else 0)
        p = self.params(opts.pop("band_rows", None), opts.pop("band_count", 1), opts.pop("band_index", 0), flags, opts.pop("stream", None))
        n = rt_noise_params()
        n.min_spp, n.step_spp, n.dilate = int(opts.pop("min_spp", 0)), int(opts.pop("step_spp", 0)), int(opts.pop("dilate", 0))
        n.rel_tol, n.lum_floor = float(opts.pop("rel_tol", 0.0)), float(opts.pop("lum_floor", 0.0))
        if opts:
            raise TypeError(f"run_noise_target: unknown options {sorted(opts)}")
        rows = check(lib.rt_local_rows(ctypes.byref(p), None), "rt_local_rows")
        npix = rows * self.width
        ptr, dev = _pointer(output_image, 3 * npix, "output_image")
        acc_ptr, acc_dev = (None, None) if accum is None else _f64(accum, "accum", 3 * npix)
        mom_ptr, mom_dev = (None, None) if moments is None else _f64(moments, "moments", 2 * npix)
        cnt_ptr, cnt_dev = (None, None) if counts is None else address(counts, "counts", ("int32",), at_least=npix)
        if same_place(output_image=dev, accum=acc_dev, counts=cnt_dev, moments=mom_dev):
            p.flags |= RT_OUT_DEVICE
        ptrs = [None if a is None else ctypes.c_void_p(a) for a in (acc_ptr, mom_ptr)]
        cnt_ptr = None if cnt_ptr is None else ctypes.c_void_p(cnt_ptr)
        st, res = rt_stats(), rt_noise_result()
        check(lib.rt_render_noise_target(self._scene, ctypes.byref(self.cam.c), ctypes.byref(p), ctypes.byref(n), ctypes.c_void_p(ptr), ptrs[0],
                                         cnt_ptr, ptrs[1], ctypes.byref(st), ctypes.byref(res)), "engine.run_noise_target")
        self.stats = st.as_dict()
        return dict(res.as_dict(), ms=st.ms)

    def run_progressive(self, output_image, callback, accum=None, samples_per_pass=0):
        """Progressive render (rt_render_progressive): the frame is traced in passes of samples_per_pass samples
        (0: spp / 8); after each pass callback(samples_done, spp) runs with output_image (and accum) holding the frame
        of the samples so far.  A truthy return value stops the render.  Returns elapsed ms, or -1 on an empty world."""
        if self._scene is None:
            print("Invalid input scene!")
            return -1
        if self.m in (engine_mode.adaptive, engine_mode.parallel_images):
            raise ValueError("progressive rendering traces whole frames of consecutive samples "
                             "(engine_mode.adaptive / parallel_images are not progressive)")
        p = self.params(None, 1, 0, 0, None)
        p.samples_per_pass = int(samples_per_pass)
        nbytes = self.height * self.width * 3
        ptr, dev = _pointer(output_image, nbytes, "output_image")
        acc_ptr, acc_dev = (None, None) if accum is None else address(accum, "accum", ANY, min_bytes=nbytes * 8)
        if same_place(output_image=dev, accum=acc_dev):
            p.flags |= RT_OUT_DEVICE
        errors = []

        def trampoline(_user, done, spp, _rgb, _acc):
            try:
                return 1 if callback(int(done), int(spp)) else 0
            except BaseException as e:  # an exception must not unwind through the C frames: stop and re-raise after
                errors.append(e)
                return 1

        cb = rt_progress_fn(trampoline)
        st = rt_stats()
        check(lib.rt_render_progressive(self._scene, ctypes.byref(self.cam.c), ctypes.byref(p), ctypes.c_void_p(ptr),
                                        ctypes.c_void_p(acc_ptr) if acc_ptr else None, cb, None, ctypes.byref(st)),
              "engine.run_progressive")
        if errors:
            raise errors[0]
        self.stats = st.as_dict()
        return int(round(st.ms))

    def local_rows(self, band_rows, band_count, band_index):
        p = self.params(band_rows, band_count, band_index)
        n = check(lib.rt_local_rows(ctypes.byref(p), None), "rt_local_rows")
        rows = (ctypes.c_int32 * max(n, 1))()
        lib.rt_local_rows(ctypes.byref(p), rows)
        return np.array(rows[:n], dtype=np.int64)
