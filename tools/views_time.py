#!/usr/bin/env python3
"""Times rt_render_views against a loop of rt_render calls of the same build, in one process on one GPU, on the same frames:

  A  V rt_render calls (engine.run), one per view, each writing its slice of one device buffer;
  B  one rt_render_views call over the same V cameras and seeds into a device buffer of the same shape.

The clock is the host's (time.perf_counter) around each form, with one device synchronisation at its end: what a caller
waits for, including the per-call work -- workspace reset, launches, rt_render's own wait and copy -- that is the point of
the comparison.  The forms alternate inside every round, so drift hits them alike; --warmup rounds, then --runs timed ones.
Every round checks that B's frames equal A's bit for bit (torch.equal on the RGB8 buffers).  Per scene and shape: the
median, minimum and maximum of each form, the ratio of the medians B / A, and `wins`: B's median is below A's by more than
the rounds' spread (the larger of the two forms' max - min).

Prints one JSON line (kept as profiles/render_views_time.json).

  python tools/views_time.py [--scenes 1,cow,8] [--shapes 64x128x128x16,4x1920x1080x16] [--runs 21] [--warmup 3]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def orbit(art, world, nviews, w, h):
    """nviews cameras on a circle about the vertical axis through lookat, starting at the scene's own."""
    cams = []
    dx, dy, dz = (f - t for f, t in zip(world.lookfrom, world.lookat))
    for v in range(nviews):
        a = 2.0 * math.pi * v / nviews
        eye = (world.lookat[0] + dx * math.cos(a) + dz * math.sin(a), world.lookat[1] + dy, world.lookat[2] - dx * math.sin(a) + dz * math.cos(a))
        cams.append(art.camera(eye, world.lookat, (0, 1, 0), world.vfov, w / h, world.aperture, 10.0, 0.0, 1.0))
    return cams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="1,cow,8")
    ap.add_argument("--shapes", default="64x128x128x16,4x1920x1080x16", help="comma-separated VxWxHxSPP")
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch

    import another_raytracer_amd as art
    if art.lib.rt_device_count() < 1:
        raise SystemExit("views_time: no HIP device")
    side = torch.cuda.Stream()
    result = {"tool": "views_time", "clock": "host wall time around each form, one synchronisation at its end", "runs": args.runs,
              "warmup": args.warmup, "seed": args.seed, "kernel_build_id": art._lib.kernel_build_id(), "scenes": {}}
    for scene in args.scenes.split(","):
        world = art.scene_manager().build(scene)
        result["scenes"][scene] = {}
        for shape in args.shapes.split(","):
            V, W, H, k = (int(x) for x in shape.split("x"))
            cams = orbit(art, world, V, W, H)
            seeds = [args.seed + v for v in range(V)]
            engines = []
            for v, cam in enumerate(cams):
                eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=k, seed=seeds[v])
                eng.set_scene(world.objects, world.background)
                engines.append(eng)
            ms = {"render_loop": [], "render_views": []}
            equal = True
            with torch.cuda.stream(side):
                a_rgb = torch.zeros((V, H, W, 3), dtype=torch.uint8, device="cuda")
                b_rgb = torch.zeros((V, H, W, 3), dtype=torch.uint8, device="cuda")
                segments = passes = None
                for r in range(args.warmup + args.runs):
                    side.synchronize()
                    t0 = time.perf_counter()
                    for v, eng in enumerate(engines):
                        eng.run(a_rgb[v], stream=side.cuda_stream)
                    side.synchronize()
                    t1 = time.perf_counter()
                    art.render_views(world, cams, W, H, k, seeds=seeds, out=b_rgb)
                    side.synchronize()
                    t2 = time.perf_counter()
                    equal = equal and bool(torch.equal(a_rgb, b_rgb))
                    if r == 0:  # outside the timed rounds: the counts, which need stats (and with them a wait inside the call)
                        _, st = art.render_views(world, cams, W, H, k, seeds=seeds, out=b_rgb, stats=True)
                        segments = (sum(e.stats["segments"] for e in engines), st["segments"])
                        passes = (sum(e.stats["passes"] for e in engines), st["passes"])
                    if r >= args.warmup:
                        ms["render_loop"].append(1e3 * (t1 - t0))
                        ms["render_views"].append(1e3 * (t2 - t1))
            side.synchronize()
            entry = {"views": V, "W": W, "H": H, "spp": k, "paths": V * W * H * k, "segments": segments[0], "segments_equal": segments[0] == segments[1],
                     "frames_equal_bit_for_bit": equal, "launches_of_the_path_kernel": {"render_loop": passes[0], "render_views": passes[1]}}
            for f, v in ms.items():
                entry[f] = {"ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}
            spread = max(e["ms_max"] - e["ms_min"] for e in (entry["render_loop"], entry["render_views"]))
            entry["spread_ms"] = spread
            entry["ratio_b_over_a"] = entry["render_views"]["ms"] / entry["render_loop"]["ms"]
            entry["wins"] = bool(entry["render_loop"]["ms"] - entry["render_views"]["ms"] > spread)
            result["scenes"][scene][shape] = entry
            del a_rgb, b_rgb, engines
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
