#!/usr/bin/env python3
"""Times rt_query_rays on one GPU: HIP events around --batch back-to-back queries on a side stream (ms per query = window /
batch), every buffer on the device, warm-up windows, then the median of the timed windows.  The three forms -- closest hit (with RT_Q_NO_MEDIA: the same primitives as the any-hit forms), any hit with the children sorted nearest first, any
hit in node order (option query.any_sorted 1 / 0) -- alternate inside every round, so drift hits them alike.

Two ray sets per scene at --width x --height (default 1920x1080; scenes 1 = the LDS image, cow, 8):
  primary  the pixel-centre rays of rt_render_guides (t_max = +inf)
  ao       ambient-occlusion rays: from the guide position of every pixel that hit something, direction = normal + a seeded
           random unit vector (made with torch on the device), t_max = 0.25 * |lookfrom - lookat|

Prints one JSON line: per scene and set the ray count, the median / min / max ms and Mrays/s of each form, the any-hit
forms' speed relative to the closest search on the same rays, and whether the occlusion bytes equal the closest search's
answer (t < t_max) and each other.

  python tools/ray_query_time.py [--scenes 1,cow,8] [--width 1920] [--height 1080] [--runs 21] [--warmup 3] [--batch 16]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("closest", "any_sorted", "any_unsorted")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="1,cow,8")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16, help="queries per timed window (one window: events around this many launches)")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch

    import another_raytracer_amd as art
    if art.lib.rt_device_count() < 1:
        raise SystemExit("ray_query_time: no HIP device")
    W, H = args.width, args.height
    default_sorted = int(art.get_option("query.any_sorted"))
    side = torch.cuda.Stream()
    result = {"tool": "ray_query_time", "W": W, "H": H, "runs": args.runs, "warmup": args.warmup, "batch": args.batch, "seed": args.seed,
              "kernel_build_id": art._lib.kernel_build_id(), "default_any_sorted": default_sorted, "scenes": {}}

    def measure(objects, rays, t_max):
        n = int(rays.shape[0])
        hits = torch.empty((n, 12), dtype=torch.float64, device="cuda")
        occ = {f: torch.empty((n,), dtype=torch.uint8, device="cuda") for f in FORMS[1:]}
        ms = {f: [] for f in FORMS}
        with torch.cuda.stream(side):
            for r in range(args.warmup + args.runs):
                for f in FORMS:
                    if f != "closest":
                        art.set_option("query.any_sorted", 1 if f == "any_sorted" else 0)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(side)
                    for _ in range(args.batch):
                        if f == "closest":
                            art.query_rays(objects, rays, t_max=t_max, no_media=True, out=hits, stream=side)
                        else:
                            art.query_rays(objects, rays, t_max=t_max, any_hit=True, out=occ[f], stream=side)
                    b.record(side)
                    b.synchronize()
                    if r >= args.warmup:
                        ms[f].append(a.elapsed_time(b) / args.batch)
        art.set_option("query.any_sorted", default_sorted)
        side.synchronize()
        want = torch.isfinite(hits[:, 0])  # the closest search stopped at t_max: a finite t is a hit inside the interval
        out = {"rays": n, "occluded_fraction": float(want.double().mean())}
        for f in FORMS:
            med = statistics.median(ms[f])
            out[f] = {"ms": med, "ms_min": min(ms[f]), "ms_max": max(ms[f]), "mrays_per_s": n / med / 1e3}
        for f in FORMS[1:]:
            out[f]["speed_vs_closest"] = out["closest"]["ms"] / out[f]["ms"]
            out[f]["equals_closest_search"] = bool((occ[f].bool() == want).all())
        out["any_forms_agree"] = bool((occ["any_sorted"] == occ["any_unsorted"]).all())
        return out

    for scene in args.scenes.split(","):
        world = art.scene_manager().build(scene)
        cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
        eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=1)
        eng.set_scene(world.objects, world.background)
        guides = torch.zeros((H, W, 10), dtype=torch.float64, device="cuda")
        prim = torch.zeros((H, W, 7), dtype=torch.float64, device="cuda")
        eng.render_guides(guides=guides, rays=prim)
        g = guides.reshape(-1, 10)
        hit = torch.isfinite(g[:, 9])
        gen = torch.Generator(device="cuda").manual_seed(args.seed)
        v = torch.randn((int(hit.sum()), 3), dtype=torch.float64, device="cuda", generator=gen)
        v = v / v.norm(dim=1, keepdim=True)
        ao = torch.cat([g[hit, 6:9], g[hit, 3:6] + v, torch.zeros((v.shape[0], 1), dtype=torch.float64, device="cuda")], dim=1).contiguous()
        reach = 0.25 * math.dist(world.lookfrom, world.lookat)
        ao_tmax = torch.full((ao.shape[0],), reach, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        result["scenes"][scene] = {"primary": measure(world.objects, prim.reshape(-1, 7), None), "ao_t_max": reach,
                                   "ao": measure(world.objects, ao, ao_tmax)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
