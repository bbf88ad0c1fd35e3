#!/usr/bin/env python3
"""Times rt_radiance_grad against rt_radiance_rays of the same build on one GPU, on the same paths: device buffers holding
rt_camera_rays of a frame with their RNG states, one ray per (pixel, sample), positive random weights.

  A  rt_radiance_rays (spp 1): rt_stats.ms spans the path kernel;
  B  rt_radiance_grad (spp 1) with all four outputs: rt_stats.ms spans the path kernel with its vertex records and walks
     back, and the kernel that rounds the accumulators.  The accumulators' memset precedes the timed region.

Both trace the same segments (checked on the first round: equal counts, radiance equal bit for bit; and B's gradients of
the first two rounds are equal bit for bit).  The forms alternate inside every round, so drift hits them alike; --warmup
rounds, then the medians of --runs rounds.

Prints one JSON line: per case the segments, the median / min / max ms of each form and the ratio B / A.

  python tools/radiance_grad_time.py [--cases 1:1920x1080x16,6:1920x1080x16,8:1920x1080x16,cow:1920x1080x16,1:256x144x16] [--runs 11] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = "1:1920x1080x16,6:1920x1080x16,8:1920x1080x16,cow:1920x1080x16,1:256x144x16"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES, help="scene:WxHxspp, comma-separated")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-depth", type=int, default=50)
    args = ap.parse_args()

    import torch

    import another_raytracer_amd as art
    if art.lib.rt_device_count() < 1:
        raise SystemExit("radiance_grad_time: no HIP device")
    side = torch.cuda.Stream()
    result = {"tool": "radiance_grad_time", "runs": args.runs, "warmup": args.warmup, "seed": args.seed, "max_depth": args.max_depth,
              "kernel_build_id": art._lib.kernel_build_id(), "cases": {}}
    for case in args.cases.split(","):
        scene, size = case.split(":")
        W, H, k = (int(x) for x in size.split("x"))
        world = art.scene_manager().build(scene)
        cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
        ms = {"radiance_rays": [], "radiance_grad": []}
        with torch.cuda.stream(side):
            rays, rng = art.camera_rays(cam, W, H, k, seed=args.seed, device=0)
            n = W * H * k
            gen = torch.Generator(device="cuda").manual_seed(7)
            weights = 0.25 + 0.75 * torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=gen)
            out_a = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            out_b = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            segments = same_radiance = same_grads = first = None
            for r in range(args.warmup + args.runs):
                _, st_a = art.radiance_rays(world, rays, rng=rng, spp=1, max_depth=args.max_depth, out=out_a, stats=True)
                _, gt, gm, gb, st_b = art.radiance_grad(world, rays, weights, rng=rng, spp=1, max_depth=args.max_depth, out_radiance=out_b, stats=True)
                grads = torch.cat([gt.reshape(-1), gm.reshape(-1), gb]).view(torch.int64)
                if r == 0:
                    same_radiance = bool(torch.equal(out_a.view(torch.int64), out_b.view(torch.int64)))
                    segments = (st_a["segments"], st_b["segments"])
                    first = grads.clone()
                elif r == 1:
                    same_grads = bool(torch.equal(first, grads))
                if r >= args.warmup:
                    ms["radiance_rays"].append(st_a["ms"])
                    ms["radiance_grad"].append(st_b["ms"])
        side.synchronize()
        entry = {"paths": n, "segments": segments[0], "segments_equal": segments[0] == segments[1], "radiance_equal_bit_for_bit": same_radiance,
                 "gradients_equal_across_runs": same_grads, "textures": int(gt.shape[0]), "materials": int(gm.shape[0])}
        for f, v in ms.items():
            med = statistics.median(v)
            entry[f] = {"ms": med, "ms_min": min(v), "ms_max": max(v), "segments_per_ms": segments[0] / med}
        entry["ratio_grad_over_rays"] = entry["radiance_grad"]["ms"] / entry["radiance_rays"]["ms"]
        result["cases"][case] = entry
        del rays, rng, weights, out_a, out_b
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
