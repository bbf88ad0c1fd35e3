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
import numpy as np

import _update_timing as ut


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


def main():
    art, torch, args, (W, H, k), result = ut.start("refit_time", "meshes", "cow,dino,9", 21, {
        "update_device_ms": "HIP events around the update's kernels", "update_wall_ms": "host wall time of update_triangles(timing=True)"})
    for name in args.meshes.split(","):
        p0 = art.scene_triangles(art.scene_manager().build(name))
        p1 = twist(p0)
        lo, hi, c, ext = box_of(p1)
        render = ut.renderer(art, art.camera((c[0] + 0.4 * ext, c[1] + 0.9 * ext, c[2] + 2.2 * ext), tuple(c), (0, 1, 0), 40.0, W / H, 0.0, 10.0, 0.0, 1.0), (W, H, k))
        a, c_same, d = (ut.compiled(art, graph_of(art, p0, p1)) for _ in range(3))
        nodes, refs = art.scene_bvh(a)
        t_p0, t_p1 = torch.from_numpy(np.array(p0)).cuda(), torch.from_numpy(p1).cuda()
        torch.cuda.synchronize()
        equal_twisted = equal_same = True
        kernel = None
        ms, rate = {}, {}
        for r in range(args.warmup + args.runs):
            m, b, w = ut.update_then_fresh(art, lambda: art.update_triangles(a, t_p1, timing=True), lambda: graph_of(art, p1, p1))
            img_a, rate_a, st = render(a)
            img_b, rate_b, _ = render(b)
            m["update_same_device_ms"] = art.update_triangles(c_same, t_p0, timing=True)
            img_c, rate_c, _ = render(c_same)
            img_d, rate_d, _ = render(d)
            art.update_triangles(a, t_p0)  # back to P0: the next round's update is this round's
            torch.cuda.synchronize()
            equal_twisted = equal_twisted and bool((img_a == img_b).all())
            equal_same = equal_same and bool((img_c == img_d).all())
            kernel = [st["kernel_features"], st["kernel_textures"], st["kernel_lds_mode"]]
            del b, w
            ut.record(args, r, ms, m, rate, {"refit_twisted": rate_a, "fresh_twisted": rate_b, "refit_same": rate_c, "fresh_same": rate_d})
        entry = {"triangles": int(len(p0)), "bvh_nodes": int(len(nodes)), "leaf_slots": int(len(refs)), "kernel": kernel,
                 "frames_equal_bit_for_bit": {"twisted": equal_twisted, "unchanged": equal_same}}
        result["meshes"][name] = ut.finish(entry, ms, rate, [("refit_twisted", "fresh_twisted", "refit", "_twisted"), ("refit_same", "fresh_same", "refit", "_unchanged")])
        del a, c_same, d
        torch.cuda.empty_cache()
    ut.report(result)


if __name__ == "__main__":
    main()
