#!/usr/bin/env python3
"""Times rt_render_noise_target on one GPU (HIP events: rt_stats.ms), a warm-up, then the median of the timed runs, with
every buffer on the device.  Prints one JSON line per mode:

  (default)   the render at the given parameters: ms, rounds, mean spp, converged share, segments; with --rmse also the
              display RMSE against a --ref-spp render (seed 99), the same for a uniform rt_render at ceil(mean spp), and
              the uniform time at equal RMSE under the 1 / sqrt(spp) model: spp_eq = spp_u * (rmse_u / rmse_nt)^2,
              ms_eq = ms_u * spp_eq / spp_u
  --overhead  the machinery alone: rel_tol = 1e-300, so every pixel with a positive variance runs to the cap through
              list-mode rounds, against rt_render at spp = cap in the same process (ratio of the medians, and of the
              segment rates, which is the fair one where zero-variance pixels retire early); and the fixed cost of a
              round (select kernel + 4-byte read-back + launch tail) from two step sizes that reach the same counts in
              different numbers of rounds: (ms_a - ms_b) / (rounds_a - rounds_b)
  --sweep     min_spp = step_spp in {8, 16, 32} x rel_tol in {0.02, 0.05, 0.1} (x dilate 0, 1): the default mode's line
              for each

  python tools/noise_target_time.py [--scene 1] [--width 1920] [--height 1080] [--cap 256] [--min-spp 32] [--step-spp 32]
                                    [--rel-tol 0.05] [--dilate 0] [--runs 5] [--warmup 1] [--rmse] [--overhead] [--sweep]
"""
import argparse
import json
import math
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
    ap.add_argument("--cap", type=int, default=256)
    ap.add_argument("--min-spp", type=int, default=32)
    ap.add_argument("--step-spp", type=int, default=32)
    ap.add_argument("--rel-tol", type=float, default=0.05)
    ap.add_argument("--dilate", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rmse", action="store_true")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--overhead", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()

    import torch

    import another_raytracer_amd as art
    if art.lib.rt_device_count() < 1:
        raise SystemExit("noise_target_time: no HIP device")
    W, H = args.width, args.height
    world = art.scene_manager().build(args.scene)
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
    count = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    base = {"scene": args.scene, "W": W, "H": H, "runs": args.runs, "warmup": args.warmup, "kernel_build_id": art._lib.kernel_build_id()}

    def engine(spp, seed):
        eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=spp, seed=seed)
        eng.set_scene(world.objects, world.background)
        return eng

    def med(values):
        return {"ms": statistics.median(values), "ms_min": min(values), "ms_max": max(values)}

    def uniform(spp, seed, runs=None):
        eng = engine(spp, seed)
        ms = []
        for r in range(args.warmup + (runs or args.runs)):
            eng.run(rgb, accum=acc)
            if r >= args.warmup:
                ms.append(eng.stats["ms"])
        return dict(med(ms), spp=spp, segments=eng.stats["segments"])

    def noise(cap, **opts):
        eng = engine(cap, args.seed)
        ms = []
        for r in range(args.warmup + args.runs):
            res = eng.run_noise_target(rgb, accum=acc, counts=count, **opts)
            if r >= args.warmup:
                ms.append(res["ms"])
        return dict(med(ms), cap=cap, rounds=res["rounds"], mean_spp=res["samples"] / (W * H), converged_share=res["converged_pixels"] / (W * H),
                    segments=eng.stats["segments"], passes=eng.stats["passes"], **opts)

    ref = None

    def display_rmse(x):
        return float(torch.sqrt(torch.mean((torch.sqrt(torch.clamp(x, 0.0, 1.0)) - torch.sqrt(torch.clamp(ref, 0.0, 1.0))) ** 2)))

    def quality(line):
        """display RMSE of the frame in acc / count, and the uniform render's at ceil(mean spp)"""
        nonlocal ref
        if ref is None:
            engine(args.ref_spp, 99).run(rgb, accum=acc)
            ref = acc / float(args.ref_spp)
        eng = engine(line["cap"], args.seed)
        eng.run_noise_target(rgb, accum=acc, counts=count, **{k: line[k] for k in ("min_spp", "step_spp", "rel_tol", "dilate")})
        line["rmse"] = display_rmse(acc / count[..., None].to(torch.float64))
        spp_u = math.ceil(line["mean_spp"])
        u = uniform(spp_u, args.seed, runs=3)
        u["rmse"] = display_rmse(acc / float(spp_u))
        spp_eq = spp_u * (u["rmse"] / line["rmse"]) ** 2
        line["uniform"] = u
        line["uniform_equal_rmse"] = {"spp": spp_eq, "ms": u["ms"] * spp_eq / spp_u, "speedup": u["ms"] * spp_eq / spp_u / line["ms"]}
        return line

    if args.overhead:
        cap = args.cap
        u = uniform(cap, args.seed)
        a = noise(cap, min_spp=args.min_spp, step_spp=args.step_spp, rel_tol=1e-300, dilate=0)
        big = cap - args.min_spp  # one round to the cap
        b = noise(cap, min_spp=args.min_spp, step_spp=big, rel_tol=1e-300, dilate=0)
        rate = lambda x: x["segments"] / x["ms"]  # noqa: E731
        print(json.dumps(dict(base, tool="noise_target_time", mode="overhead", uniform=u, many_rounds=a, one_round=b,
                              ms_ratio=a["ms"] / u["ms"], segment_rate_ratio=rate(a) / rate(u), one_round_segment_rate_ratio=rate(b) / rate(u),
                              per_round_fixed_ms=(a["ms"] - b["ms"]) / (a["rounds"] - b["rounds"]) if a["rounds"] != b["rounds"] else None)))
        return
    if args.sweep:
        for dilate in (0, 1):
            for m in (8, 16, 32):
                for tol in (0.02, 0.05, 0.1):
                    line = noise(args.cap, min_spp=m, step_spp=m, rel_tol=tol, dilate=dilate)
                    print(json.dumps(dict(base, tool="noise_target_time", mode="sweep", **quality(line))), flush=True)
        return
    line = noise(args.cap, min_spp=args.min_spp, step_spp=args.step_spp, rel_tol=args.rel_tol, dilate=args.dilate)
    if args.rmse:
        line = quality(line)
    print(json.dumps(dict(base, tool="noise_target_time", mode="render", **line)))


if __name__ == "__main__":
    main()
