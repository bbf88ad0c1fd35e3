#!/usr/bin/env python3
"""Times rt_scene_update_materials + rt_scene_update_textures against what the library offered before them -- a fresh
compile and upload of the same values -- and checks that a recoloured scene renders at the fresh compile's rate, in one
process on one GPU.  The scenes are tools/sphere_update_time.py's:
  spheres  scene 1's spheres with a palette of 64 seeded materials in one bvh_node: runs k_paths out of the LDS scene
           image, so the update includes the image's shading table;
  mixed    the cow's triangles and 256 spheres above them in one bvh_node, and a loose sphere light (k_paths_g).
V1 gives every solid colour, metal and dielectric new seeded values: colours and albedos in [0.05, 0.95]^3 (a light's
colour in [1, 8]^3), fuzz in [0, 0.6], ir in [1.2, 2.4].

Every round:
  (i)  scene A (compiled with V0) is updated to V1 from two device tensors (materials, then textures): the device time of
       the two calls' kernels (HIP events, summed) and the host wall time of the two calls; scene B is compiled fresh with
       V1 and uploaded: host wall time of rt_graph_compile + the upload (the Python calls that rebuild the graph are timed
       apart and not counted).
  (ii) A and B render W x H x spp: segments per millisecond of device time; the frames must be equal bit for bit
       (asserted every round).
A goes back to V0 before the next round, so every timed update is the same one.  --warmup rounds, then --runs timed
ones; medians, minima and maxima, the ratios of the medians, and whether a difference exceeds the rounds' spread.

Prints one JSON line (kept as profiles/material_update_time.json).

  python tools/material_update_time.py [--scenes spheres,mixed] [--shape 1920x1080x16] [--runs 15] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sphere_update_time import SKY, compiled, mixed_scene, spheres_scene, summary  # noqa: E402

LAMBERTIAN, METAL, DIELECTRIC, LIGHT = 0, 1, 2, 3
SOLID = 0


class WithValues:
    """The package with its material constructors taking their values from M / T by running id (a compiled index is the
    graph's id), so that sphere_update_time's graph functions build the same call sequence with other values."""

    def __init__(self, art, M, T):
        self._art, self._M, self._T, self._nm, self._nt = art, M, T, 0, 0

    def __getattr__(self, name):
        return getattr(self._art, name)

    def reset_scene_rng(self):
        self._nm = self._nt = 0
        self._art.reset_scene_rng()

    def _colour(self):  # a colour argument makes one solid texture
        c = tuple(float(x) for x in self._T[self._nt, :3])
        self._nt += 1
        return c

    def lambertian(self, colour):
        self._nm += 1
        return self._art.lambertian(self._colour())

    def diffuse_light(self, colour):
        self._nm += 1
        return self._art.diffuse_light(self._colour())

    def metal(self, albedo, fuzz):
        row = self._M[self._nm]
        self._nm += 1
        return self._art.metal(tuple(float(x) for x in row[:3]), float(row[3]))

    def dielectric(self, ir):
        row = self._M[self._nm]
        self._nm += 1
        return self._art.dielectric(float(row[4]))


def new_values(M0, Md, T0, Td, seed=4):
    rng = np.random.default_rng(seed)
    M, T = np.array(M0), np.array(T0)
    lit = {int(t) for ty, t in Md if ty == LIGHT}
    for k, (ty, _, _) in enumerate(Td):
        if ty == SOLID:
            T[k, :3] = rng.uniform(1.0, 8.0, 3) if k in lit else rng.uniform(0.05, 0.95, 3)
    for k, (ty, _) in enumerate(Md):
        if ty == METAL:
            M[k, :3], M[k, 3] = rng.uniform(0.05, 0.95, 3), rng.uniform(0.0, 0.6)
        elif ty == DIELECTRIC:
            M[k, 4] = rng.uniform(1.2, 2.4)
    return M, T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="spheres,mixed")
    ap.add_argument("--shape", default="1920x1080x16", help="WxHxSPP of the rendered frames")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    import another_raytracer_amd as art
    if art.lib.rt_device_count() < 1:
        raise SystemExit("material_update_time: no HIP device")
    W, H, k = (int(x) for x in args.shape.split("x"))
    result = {"tool": "material_update_time", "runs": args.runs, "warmup": args.warmup, "W": W, "H": H, "spp": k,
              "clock": {"update_device_ms": "HIP events around each call's kernels, update_materials + update_textures",
                        "update_wall_ms": "host wall time of the two calls (timing=True: each waits)",
                        "fresh_compile_upload_ms": "host wall time of rt_graph_compile + the upload", "render": "segments / rt_stats.ms (HIP events)"},
              "kernel_build_id": art._lib.kernel_build_id(), "scenes": {}}
    for name in args.scenes.split(","):
        s0, graph0, (lookfrom, lookat, vfov) = {"spheres": spheres_scene, "mixed": mixed_scene}[name](art)
        a = compiled(art, graph0(s0))
        (M0, Md), (T0, Td) = art.scene_materials(a), art.scene_textures(a)
        M1, T1 = new_values(M0, Md, T0, Td)
        # the same graph function over the package with V1 in its constructors
        _, graph1, _ = {"spheres": spheres_scene, "mixed": mixed_scene}[name](WithValues(art, M1, T1))
        cam = art.camera(lookfrom, lookat, (0, 1, 0), vfov, W / H, 0.0, 10.0, 0.0, 1.0)

        def render(world):
            eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=k, seed=1)
            eng.set_scene(world, SKY)
            img = np.zeros((H, W, 3), np.uint8)
            eng.run(img)
            return img, eng.stats["segments"] / eng.stats["ms"], eng.stats

        has_image = art.scene_lds_image(a) is not None
        img_v0 = render(a)[0]
        dev = [torch.from_numpy(np.array(x)).cuda() for x in (M0, T0, M1, T1)]
        torch.cuda.synchronize()
        ms = {f: [] for f in ("update_device_ms", "update_wall_ms", "graph_python_ms", "fresh_compile_upload_ms")}
        rate = {f: [] for f in ("updated", "fresh")}
        kernel = None
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            dev_ms = art.update_materials(a, dev[2], timing=True) + art.update_textures(a, dev[3], timing=True)
            t1 = time.perf_counter()
            w = graph1(s0)
            t2 = time.perf_counter()
            b = compiled(art, w)
            t3 = time.perf_counter()
            img_a, rate_a, st = render(a)
            img_b, rate_b, _ = render(b)
            assert (img_a == img_b).all(), f"{name}, round {r}: the updated scene's frame differs from the fresh compile's"
            assert (img_a != img_v0).any(), f"{name}: the update is not visible"
            if r == 0:
                assert (art.scene_materials(b)[0].view(np.int64) == M1.view(np.int64)).all() and (art.scene_textures(b)[0].view(np.int64) == T1.view(np.int64)).all()
            art.update_materials(a, dev[0])  # back to V0: the next round's update is this round's
            art.update_textures(a, dev[1])
            torch.cuda.synchronize()
            kernel = [st["kernel_features"], st["kernel_textures"], st["kernel_lds_mode"], st["extend_variant"]]
            del b, w
            if r < args.warmup:
                continue
            for f, v in (("update_device_ms", dev_ms), ("update_wall_ms", 1e3 * (t1 - t0)), ("graph_python_ms", 1e3 * (t2 - t1)),
                         ("fresh_compile_upload_ms", 1e3 * (t3 - t2))):
                ms[f].append(v)
            rate["updated"].append(rate_a)
            rate["fresh"].append(rate_b)
        entry = {"materials": int(len(M0)), "textures": int(len(T0)), "metals": int((Md[:, 0] == METAL).sum()), "dielectrics": int((Md[:, 0] == DIELECTRIC).sum()),
                 "solid_colours": int((Td[:, 0] == SOLID).sum()), "lds_image": has_image, "kernel": kernel, "frames_equal_bit_for_bit": True}
        entry.update({f: summary(v) for f, v in ms.items()})
        entry["segments_per_ms"] = {f: summary(v) for f, v in rate.items()}
        entry["update_device_over_fresh"] = entry["update_device_ms"]["median"] / entry["fresh_compile_upload_ms"]["median"]
        entry["update_wall_over_fresh"] = entry["update_wall_ms"]["median"] / entry["fresh_compile_upload_ms"]["median"]
        entry["update_is_faster"] = bool(entry["update_wall_ms"]["max"] < entry["fresh_compile_upload_ms"]["min"])
        sx, sy = entry["segments_per_ms"]["updated"], entry["segments_per_ms"]["fresh"]
        spread = max(sx["max"] - sx["min"], sy["max"] - sy["min"])
        entry["render_rate_updated_over_fresh"] = sx["median"] / sy["median"]
        entry["render_rate_difference_exceeds_spread"] = bool(abs(sx["median"] - sy["median"]) > spread)
        result["scenes"][name] = entry
        del a
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
