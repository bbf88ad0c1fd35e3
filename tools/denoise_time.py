#!/usr/bin/env python3
"""Times rt_denoise on one GPU: HIP events around the filter kernels (rt_denoise's `ms`), a warm-up, then the median of
the timed runs, with every buffer on the device.  Default: 1920x1080, 5 iterations, on two 2-spp half-renders of a
builtin scene and its guides.  Prints one JSON line:

  ms                      median of the whole filter (prepare + iterations + finish)
  by_iterations           median ms with 1 .. N iterations (the difference of neighbours is one iteration's time)
  forms                   the first two iterations (tap spacings 1, 2) as LDS-tile and as direct-load kernels
                          (option denoise.lds_iterations 2 / 1 / 0), whole filter and the iteration alone
  compulsory_ms_per_iter  120 B per pixel (reads 24 L + 8 V + 56 normal/position/t, writes 24 + 8) at --stream-tbs
  compulsory_fraction     compulsory time of all iterations / (ms of N iterations - ms of the 0-iteration remainder)

  python tools/denoise_time.py [--scene 1] [--width 1920] [--height 1080] [--iterations 5] [--runs 21] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="1")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stream-tbs", type=float, default=6.3, help="streaming bandwidth the compulsory time is taken at, TB/s")
    args = ap.parse_args()

    import torch

    import another_raytracer_amd as art
    if art.lib.rt_device_count() < 1:
        raise SystemExit("denoise_time: no HIP device")
    W, H = args.width, args.height
    world = art.scene_manager().build(args.scene)
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    halves = []
    for seed in (1, 2):
        eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=2, seed=seed)
        eng.set_scene(world.objects, world.background)
        rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        acc = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
        eng.run(rgb, accum=acc)
        halves.append(acc)
    guides = torch.zeros((H, W, 10), dtype=torch.float64, device="cuda")
    eng.render_guides(guides=guides)
    out = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")

    def timed(iterations, lds_iterations):
        art.set_option("denoise.lds_iterations", lds_iterations)
        ms = []
        for r in range(args.warmup + args.runs):
            _, t = art.denoise(halves[0], halves[1], 2, guides, out_color=out, iterations=iterations)
            if r >= args.warmup:
                ms.append(t)
        return statistics.median(ms), min(ms), max(ms)

    default_lds = int(art.get_option("denoise.lds_iterations"))
    by_iter = {}
    for n in range(1, args.iterations + 1):
        by_iter[n] = timed(n, default_lds)[0]
    med, lo, hi = timed(args.iterations, default_lds)
    forms = {}
    for lds in (2, 1, 0):
        forms[f"lds_iterations_{lds}"] = {"ms": timed(args.iterations, lds)[0], "one_iteration_ms": timed(1, lds)[0],
                                          "two_iterations_ms": timed(2, lds)[0] if args.iterations >= 2 else None}
    art.set_option("denoise.lds_iterations", default_lds)
    npix = W * H
    bytes_per_iter = 120 * npix
    comp_ms = bytes_per_iter / (args.stream_tbs * 1e12) * 1e3
    # the part of one call that is not an iteration: prepare + finish = ms(1) - (ms(2) - ms(1)) when there are two
    iter_ms = med - (by_iter[1] - (by_iter[2] - by_iter[1])) if args.iterations >= 2 else med
    print(json.dumps({
        "tool": "denoise_time", "scene": args.scene, "W": W, "H": H, "iterations": args.iterations, "runs": args.runs, "warmup": args.warmup,
        "kernel_build_id": art._lib.kernel_build_id(), "default_lds_iterations": default_lds,
        "ms": med, "ms_min": lo, "ms_max": hi, "by_iterations": by_iter, "forms": forms,
        "bytes_per_iteration": bytes_per_iter, "stream_tbs": args.stream_tbs, "compulsory_ms_per_iter": comp_ms,
        "iterations_ms": iter_ms, "compulsory_fraction": args.iterations * comp_ms / iter_ms if iter_ms > 0 else None,
    }))


if __name__ == "__main__":
    main()
