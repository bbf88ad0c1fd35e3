"""What tools/refit_time.py, sphere_update_time.py and material_update_time.py share: each times an update of a compiled
scene against a fresh compile and upload of the same values, then the render rates of the two, over --warmup + --runs
rounds in one process on one GPU, and prints one JSON line.  A tool keeps its scenes, its new values and what it does
in a round; the arguments, the timers, the rounds' bookkeeping, the summaries, the ratios and the spread verdicts are here."""
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


def start(tool, things, default, runs, clock):
    """The tool's arguments (--<things> <default>, --shape, --runs, --warmup), the package on a device, and the result's
    head: (art, torch, args, (W, H, spp), result); result[things] takes one entry per scene."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--" + things, default=default)
    ap.add_argument("--shape", default="1920x1080x16", help="WxHxSPP of the rendered frames")
    ap.add_argument("--runs", type=int, default=runs)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    import another_raytracer_amd as art
    if art.lib.rt_device_count() < 1:
        raise SystemExit(f"{tool}: no HIP device")
    W, H, k = (int(x) for x in args.shape.split("x"))
    clock = dict(clock, fresh_compile_upload_ms="host wall time of rt_graph_compile + the upload", render="segments / rt_stats.ms (HIP events)")
    result = {"tool": tool, "runs": args.runs, "warmup": args.warmup, "W": W, "H": H, "spp": k, "clock": clock,
              "kernel_build_id": art._lib.kernel_build_id(), things: {}}
    return art, torch, args, (W, H, k), result


def compiled(art, w, upload=True):
    h = art.hittable_list(native=art.compile_world(w, 0))
    if upload:
        n = ctypes.c_int64()
        art._lib.check(art.lib.rt_scene_bvh_get(h._native, None, 0, None, 0, ctypes.byref(n), None), "upload")
    return h


def renderer(art, cam, shape):
    """render(world) -> (frame, segments per ms of device time, stats) at the tool's shape through cam."""
    W, H, k = shape

    def render(world):
        eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=k, seed=1)
        eng.set_scene(world, SKY)
        img = np.zeros((H, W, 3), np.uint8)
        eng.run(img)
        return img, eng.stats["segments"] / eng.stats["ms"], eng.stats
    return render


def update_then_fresh(art, update, graph):
    """A round's timed part: update() (returns the device time of its kernels) with its host wall time, then graph() --
    the Python calls that rebuild the graph, timed apart -- and its compile and upload.  Returns (the four times in ms,
    the fresh scene, its graph).  A tool's round stays inline in its loop and deletes only these two when it ends: dropping
    the round's frames as well right before the next timed update (a round in a function of its own does) was measured
    to add 15-100 us to update_wall_ms."""
    t0 = time.perf_counter()
    dev_ms = update()
    t1 = time.perf_counter()
    w = graph()
    t2 = time.perf_counter()
    b = compiled(art, w)
    t3 = time.perf_counter()
    return {"update_device_ms": dev_ms, "update_wall_ms": 1e3 * (t1 - t0), "graph_python_ms": 1e3 * (t2 - t1), "fresh_compile_upload_ms": 1e3 * (t3 - t2)}, b, w


def record(args, r, ms, m, rate, q):
    """Round r's times m and render rates q (by field) into the lists ms and rate, unless r is a warm-up round."""
    if r < args.warmup:
        return
    for into, vals in ((ms, m), (rate, q)):
        for f, v in vals.items():
            into.setdefault(f, []).append(v)


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def finish(entry, ms, rate, compared):
    """The entry's figures: every field's summary, the update over the fresh compile (ratios of the medians; faster when
    its slowest round beats the compile's fastest), and for each (x, y, name, suffix) of `compared` the render rate x over
    y with whether the medians differ by more than either's spread over the rounds."""
    entry.update({f: summary(v) for f, v in ms.items()})
    entry["segments_per_ms"] = {f: summary(v) for f, v in rate.items()}
    entry["update_device_over_fresh"] = entry["update_device_ms"]["median"] / entry["fresh_compile_upload_ms"]["median"]
    entry["update_wall_over_fresh"] = entry["update_wall_ms"]["median"] / entry["fresh_compile_upload_ms"]["median"]
    entry["update_is_faster"] = bool(entry["update_wall_ms"]["max"] < entry["fresh_compile_upload_ms"]["min"])
    for x, y, name, suffix in compared:
        sx, sy = entry["segments_per_ms"][x], entry["segments_per_ms"][y]
        spread = max(sx["max"] - sx["min"], sy["max"] - sy["min"])
        entry[f"render_rate_{name}_over_fresh{suffix}"] = sx["median"] / sy["median"]
        entry["render_rate_difference_exceeds_spread" + suffix] = bool(abs(sx["median"] - sy["median"]) > spread)
    return entry


def report(result):
    print(json.dumps(result))
