#!/usr/bin/env python3
"""Times rt_radiance_grad_texels against rt_radiance_grad of the same build on one GPU, on the same paths, and
rt_scene_update_texels of a whole image against compiling and uploading the scene anew.  Device buffers holding
rt_camera_rays of a frame with their RNG states, one ray per (pixel, sample), positive random weights.

  A  rt_radiance_grad (spp 1), four outputs: its kernels are the parent's bytes, so it is the yardstick;
  B  rt_radiance_grad_texels (spp 1), five outputs: rt_stats.ms spans the texel table's zeroing, k_texel_grad,
     k_grad_finish and k_texel_finish (A's spans k_radiance_grad and k_grad_finish: its small table's memset precedes
     the timed region).
  U  rt_scene_update_texels of image 0, all rows, from a device tensor: the device time (ms) and the wall time of the
     call with a wait;
  C  the wall time of scene_manager().build(scene) plus the first call on the new scene (the upload), --compiles times.

A and B trace the same segments (checked on the first round: equal counts, radiance and the four shared outputs equal
bit for bit; and B's texel gradients of the first two rounds are equal bit for bit).  A and B alternate inside every
round, so drift hits them alike; --warmup rounds, then the medians of --runs rounds.

Prints one JSON line: per case the texel count, the table's copies and bytes, the median / min / max ms of each form and
the ratios B / A and C / U.

  python tools/texel_grad_time.py [--cases 4:1920x1080x16,8:1920x1080x16,9:1920x1080x16,9:256x144x16] [--runs 11] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = "4:1920x1080x16,8:1920x1080x16,9:1920x1080x16,9:256x144x16"
BUDGET, ROW_BYTES, MAX_COPIES = 256 << 20, 80, 64  # csrc/launch.h: kTexelTableBudget, kGradRowLimbs * 8, kGradMaxCopies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES, help="scene:WxHxspp, comma-separated")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--compiles", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-depth", type=int, default=50)
    args = ap.parse_args()

    import numpy as np
    import torch

    import another_raytracer_amd as art
    if art.lib.rt_device_count() < 1:
        raise SystemExit("texel_grad_time: no HIP device")
    side = torch.cuda.Stream()
    result = {"tool": "texel_grad_time", "runs": args.runs, "warmup": args.warmup, "seed": args.seed, "max_depth": args.max_depth,
              "kernel_build_id": art._lib.kernel_build_id(), "cases": {}}
    one_ray = np.array([[0.0, 0.0, 10.0, 0.0, 0.0, -1.0, 0.0]])
    for case in args.cases.split(","):
        scene, size = case.split(":")
        W, H, k = (int(x) for x in size.split("x"))
        compile_ms = []
        for _ in range(args.compiles):
            t0 = time.perf_counter()
            world = art.scene_manager().build(scene)
            art.radiance_rays(world, one_ray, max_depth=1)  # the first call uploads
            compile_ms.append(1e3 * (time.perf_counter() - t0))
        cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
        desc, _, _ = art.scene_images(world)
        texels = int((desc[:, 0].astype(np.int64) * desc[:, 1]).sum())
        ms = {"radiance_grad": [], "radiance_grad_texels": [], "update_texels": [], "update_texels_wall": []}
        with torch.cuda.stream(side):
            rays, rng = art.camera_rays(cam, W, H, k, seed=args.seed, device=0)
            n = W * H * k
            gen = torch.Generator(device="cuda").manual_seed(7)
            weights = 0.25 + 0.75 * torch.rand((n, 3), dtype=torch.float64, device="cuda", generator=gen)
            out_a = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            out_b = torch.empty((n, 3), dtype=torch.float64, device="cuda")
            image = torch.from_numpy(art.scene_texels(world, 0)).to("cuda")
            segments = same_shared = same_texels = first = None
            for r in range(args.warmup + args.runs):
                _, gt, gm, gb, st_a = art.radiance_grad(world, rays, weights, rng=rng, spp=1, max_depth=args.max_depth, out_radiance=out_a, stats=True)
                _, xt, xm, xb, gx, st_b = art.radiance_grad(world, rays, weights, rng=rng, spp=1, max_depth=args.max_depth, out_radiance=out_b,
                                                            stats=True, texels=True)
                t0 = time.perf_counter()
                u_ms = art.update_texels(world, 0, image, timing=True)  # a timed call waits
                u_wall = 1e3 * (time.perf_counter() - t0)
                if r == 0:
                    shared = [torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in ((out_a, out_b), (gt, xt), (gm, xm), (gb, xb))]
                    same_shared = bool(all(shared))
                    segments = (st_a["segments"], st_b["segments"])
                    first = gx.view(torch.int64).clone()
                elif r == 1:
                    same_texels = bool(torch.equal(first, gx.view(torch.int64)))
                if r >= args.warmup:
                    ms["radiance_grad"].append(st_a["ms"])
                    ms["radiance_grad_texels"].append(st_b["ms"])
                    ms["update_texels"].append(u_ms)
                    ms["update_texels_wall"].append(u_wall)
            touched = int((gx != 0).any(1).sum())
        side.synchronize()
        copies = max(1, min(MAX_COPIES, BUDGET // (texels * ROW_BYTES)))  # (never more than the grid's blocks: not the case at these sizes)
        entry = {"paths": n, "segments": segments[0], "segments_equal": segments[0] == segments[1], "shared_outputs_equal_bit_for_bit": same_shared,
                 "texel_gradients_equal_across_runs": same_texels, "images": int(len(desc)), "texels": texels, "texels_touched": touched,
                 "image0": [int(x) for x in desc[0]], "texel_table_copies": copies, "texel_table_bytes": copies * texels * ROW_BYTES}
        for f, v in ms.items():
            entry[f] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}
        entry["compile_and_upload_wall"] = {"ms": statistics.median(compile_ms), "ms_min": min(compile_ms), "ms_max": max(compile_ms)}
        entry["ratio_texels_over_grad"] = entry["radiance_grad_texels"]["ms"] / entry["radiance_grad"]["ms"]
        entry["ratio_compile_over_update_wall"] = entry["compile_and_upload_wall"]["ms"] / entry["update_texels_wall"]["ms"]
        result["cases"][case] = entry
        del rays, rng, weights, out_a, out_b, image, gx, first
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
