#!/usr/bin/env python3
"""Times rt_radiance_rays against rt_render of the same build on one GPU, on the same paths:

  A  rt_render of the frame (device outputs): rt_stats.ms and rt_stats.segments -- its HIP events span the path kernel, the
     per-pixel sums and the RGB8 frame;
  B  rt_radiance_rays (spp 1) on device buffers holding rt_camera_rays of that frame, with their RNG states: the same paths,
     one ray per (pixel, sample) in pixel-major order; rt_stats.ms spans the path kernel.

Both trace the same segments (checked: the counts are equal and B's in-order sums equal A's out_accum bit for bit on the first
round).  What B pays that A does not: 56 + 8 B read per path (the ray and its state, where A generates them in registers),
24 B written per path to the caller's buffer, no first-bounce batches (k_paths) and no LDS copies of the BVH (k_paths_g LM 1 / 2).
The forms alternate inside every round, so drift hits them alike; --warmup rounds, then the medians of --runs rounds.

Prints one JSON line: per scene the segments, the median / min / max ms and segments per ms of each form, and the ratio B / A.

  python tools/radiance_rays_time.py [--scenes 1,cow,8] [--width 1920] [--height 1080] [--spp 16] [--runs 21] [--warmup 3]
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
    ap.add_argument("--scenes", default="1,cow,8")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch

    import another_raytracer_amd as art
    if art.lib.rt_device_count() < 1:
        raise SystemExit("radiance_rays_time: no HIP device")
    W, H, k = args.width, args.height, args.spp
    side = torch.cuda.Stream()
    result = {"tool": "radiance_rays_time", "W": W, "H": H, "spp": k, "runs": args.runs, "warmup": args.warmup, "seed": args.seed,
              "kernel_build_id": art._lib.kernel_build_id(), "scenes": {}}
    for scene in args.scenes.split(","):
        world = art.scene_manager().build(scene)
        cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
        eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=k, seed=args.seed)
        eng.set_scene(world.objects, world.background)
        ms = {"render": [], "radiance_rays": []}
        with torch.cuda.stream(side):
            img = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            acc = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
            rays, rng = art.camera_rays(cam, W, H, k, seed=args.seed, device=0)
            out = torch.empty((W * H * k, 3), dtype=torch.float64, device="cuda")
            segments = same_sums = None
            for r in range(args.warmup + args.runs):
                eng.run(img, accum=acc, stream=side.cuda_stream)
                _, st = art.radiance_rays(world, rays, rng=rng, spp=1, out=out, stats=True)
                if r == 0:
                    per = out.reshape(-1, k, 3)
                    composed = torch.zeros_like(per[:, 0])
                    for s in range(k):
                        composed = composed + per[:, s]
                    same_sums = bool(torch.equal(composed.view(torch.int64), acc.reshape(-1, 3).view(torch.int64)))
                    segments = (eng.stats["segments"], st["segments"])
                if r >= args.warmup:
                    ms["render"].append(eng.stats["ms"])
                    ms["radiance_rays"].append(st["ms"])
        side.synchronize()
        entry = {"paths": W * H * k, "segments": segments[0], "segments_equal": segments[0] == segments[1], "sums_equal_bit_for_bit": same_sums,
                 "render_kernel": [eng.stats["kernel_features"], eng.stats["kernel_textures"], eng.stats["kernel_lds_mode"]]}
        for f, v in ms.items():
            med = statistics.median(v)
            entry[f] = {"ms": med, "ms_min": min(v), "ms_max": max(v), "segments_per_ms": segments[0] / med}
        entry["ratio_b_over_a"] = entry["radiance_rays"]["segments_per_ms"] / entry["render"]["segments_per_ms"]
        result["scenes"][scene] = entry
        del rays, rng, out, img, acc
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
