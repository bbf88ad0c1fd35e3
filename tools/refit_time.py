#!/usr/bin/env python3
"""Times rt_scene_update_triangles against what the library offered before it -- a fresh compile and upload of the same
vertices -- and measures what a refitted tree costs at render time, in one process on one GPU.  The meshes are caller-built:
the triangles of a builtin scene (cow, dino, the capsule) as one solid lambertian in a bvh_node, with a sphere light.
P1 is the tests' deformation: a 90 degree twist about the vertical axis growing with height, then a 1.5 x stretch in x.

Every round:
  (i)   scene A (compiled from P0) is updated to P1 from a device tensor: the device time of the update's kernels (HIP
        events) and the host wall time of the call; scene B is compiled fresh from P1 and uploaded: host wall time of
        rt_graph_compile + the upload (the Python calls that rebuild the graph are timed apart and not counted).
  (ii)  A and B render W x H x spp: segments per millisecond of device time; the frames must be equal bit for bit.
  (iii) scene C (compiled from P0) is updated with its own vertices and renders against D, compiled from P0 and never
        updated: what the lost split-BVH clipping alone costs; the frames must be equal bit for bit.
A goes back to P0 before the next round, so every timed update is the same one.  --warmup rounds, then --runs timed
ones; medians, minima and maxima, the ratios of the medians, and whether a difference exceeds the rounds' spread.

Prints one JSON line (kept as profiles/refit_time.json).

  python tools/refit_time.py [--meshes cow,dino,9] [--shape 1920x1080x16] [--runs 21] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SKY = (0.6, 0.7, 0.9)


def box_of(p):
    lo, hi = p.reshape(-1, 3).min(0), p.reshape(-1, 3).max(0)
    return lo, hi, 0.5 * (lo + hi), float((hi - lo).max())


def twist(p):
    lo, hi, c, _ = box_of(p)
    q = p - c
    a = 0.5 * np.pi * (p[..., 1] - lo[1]) / (hi[1] - lo[1])
    x = np.cos(a) * q[..., 0] + np.sin(a) * q[..., 2]
    z = -np.sin(a) * q[..., 0] + np.cos(a) * q[..., 2]
    return np.ascontiguousarray(np.stack([1.5 * x, q[..., 1], z], -1) + c)


def graph_of(art, p, frame):
    """The world of triangles p as a hittable_list of graph objects (not yet compiled)."""
    art.reset_scene_rng()
    mat, light = art.lambertian((0.7, 0.6, 0.5)), art.diffuse_light((4.0, 4.0, 4.0))
    lo, hi, c, ext = box_of(frame)
    w = art.hittable_list()
    w.add(art.bvh_node([art.triangle(t[0], t[1], t[2], mat) for t in p]))
    w.add(art.sphere((c[0], hi[1] + 2.0 * ext, c[2]), 0.5 * ext, light))
    return w


def compiled(art, w, upload=True):
    h = art.hittable_list(native=art.compile_world(w, 0))
    if upload:
        n = ctypes.c_int64()
        art._lib.check(art.lib.rt_scene_bvh_get(h._native, None, 0, None, 0, ctypes.byref(n), None), "upload")
    return h


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="cow,dino,9")
    ap.add_argument("--shape", default="1920x1080x16", help="WxHxSPP of the rendered frames")
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    import another_raytracer_amd as art
    if art.lib.rt_device_count() < 1:
        raise SystemExit("refit_time: no HIP device")
    W, H, k = (int(x) for x in args.shape.split("x"))
    result = {"tool": "refit_time", "runs": args.runs, "warmup": args.warmup, "W": W, "H": H, "spp": k,
              "clock": {"update_device_ms": "HIP events around the update's kernels", "update_wall_ms": "host wall time of update_triangles(timing=True)",
                        "fresh_compile_upload_ms": "host wall time of rt_graph_compile + the upload", "render": "segments / rt_stats.ms (HIP events)"},
              "kernel_build_id": art._lib.kernel_build_id(), "meshes": {}}
    for name in args.meshes.split(","):
        p0 = art.scene_triangles(art.scene_manager().build(name))
        p1 = twist(p0)
        lo, hi, c, ext = box_of(p1)
        cam = art.camera((c[0] + 0.4 * ext, c[1] + 0.9 * ext, c[2] + 2.2 * ext), tuple(c), (0, 1, 0), 40.0, W / H, 0.0, 10.0, 0.0, 1.0)

        def render(world):
            eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=k, seed=1)
            eng.set_scene(world, SKY)
            img = np.zeros((H, W, 3), np.uint8)
            eng.run(img)
            return img, eng.stats["segments"] / eng.stats["ms"], eng.stats

        a, c_same, d = compiled(art, graph_of(art, p0, p1)), compiled(art, graph_of(art, p0, p1)), compiled(art, graph_of(art, p0, p1))
        nodes, refs = art.scene_bvh(a)
        t_p0, t_p1 = torch.from_numpy(np.array(p0)).cuda(), torch.from_numpy(p1).cuda()
        torch.cuda.synchronize()
        ms = {f: [] for f in ("update_device_ms", "update_wall_ms", "update_same_device_ms", "graph_python_ms", "fresh_compile_upload_ms")}
        rate = {f: [] for f in ("refit_twisted", "fresh_twisted", "refit_same", "fresh_same")}
        equal_twisted = equal_same = True
        kernel = None
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            dev_ms = art.update_triangles(a, t_p1, timing=True)
            t1 = time.perf_counter()
            w = graph_of(art, p1, p1)
            t2 = time.perf_counter()
            b = compiled(art, w)
            t3 = time.perf_counter()
            img_a, rate_a, st = render(a)
            img_b, rate_b, _ = render(b)
            same_ms = art.update_triangles(c_same, t_p0, timing=True)
            img_c, rate_c, _ = render(c_same)
            img_d, rate_d, _ = render(d)
            art.update_triangles(a, t_p0)  # back to P0: the next round's update is this round's
            torch.cuda.synchronize()
            equal_twisted = equal_twisted and bool((img_a == img_b).all())
            equal_same = equal_same and bool((img_c == img_d).all())
            kernel = [st["kernel_features"], st["kernel_textures"], st["kernel_lds_mode"]]
            del b, w
            if r < args.warmup:
                continue
            for f, v in (("update_device_ms", dev_ms), ("update_wall_ms", 1e3 * (t1 - t0)), ("update_same_device_ms", same_ms),
                         ("graph_python_ms", 1e3 * (t2 - t1)), ("fresh_compile_upload_ms", 1e3 * (t3 - t2))):
                ms[f].append(v)
            for f, v in (("refit_twisted", rate_a), ("fresh_twisted", rate_b), ("refit_same", rate_c), ("fresh_same", rate_d)):
                rate[f].append(v)
        entry = {"triangles": int(len(p0)), "bvh_nodes": int(len(nodes)), "leaf_slots": int(len(refs)), "kernel": kernel,
                 "frames_equal_bit_for_bit": {"twisted": equal_twisted, "unchanged": equal_same}}
        entry.update({f: summary(v) for f, v in ms.items()})
        entry["segments_per_ms"] = {f: summary(v) for f, v in rate.items()}
        entry["update_device_over_fresh"] = entry["update_device_ms"]["median"] / entry["fresh_compile_upload_ms"]["median"]
        entry["update_wall_over_fresh"] = entry["update_wall_ms"]["median"] / entry["fresh_compile_upload_ms"]["median"]
        entry["update_is_faster"] = bool(entry["update_wall_ms"]["max"] < entry["fresh_compile_upload_ms"]["min"])
        for tag, x, y in (("twisted", "refit_twisted", "fresh_twisted"), ("unchanged", "refit_same", "fresh_same")):
            sx, sy = entry["segments_per_ms"][x], entry["segments_per_ms"][y]
            spread = max(sx["max"] - sx["min"], sy["max"] - sy["min"])
            entry["render_rate_refit_over_fresh_" + tag] = sx["median"] / sy["median"]
            entry["render_rate_difference_exceeds_spread_" + tag] = bool(abs(sx["median"] - sy["median"]) > spread)
        result["meshes"][name] = entry
        del a, c_same, d
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
