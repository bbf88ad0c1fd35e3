#!/usr/bin/env python3
"""Times rt_scene_update_spheres against what the library offered before it -- a fresh compile and upload of the same
spheres -- and measures what a refitted sphere tree costs at render time, in one process on one GPU.  Two caller-built
scenes:
  spheres  scene 1's spheres (art.scene_spheres of the builtin scene: the ground, the small spheres, the three large
           ones) in one bvh_node with seeded materials, every 8th small sphere moving along y: a spheres-only scene that
           runs k_paths out of the LDS scene image, so the update includes the image refit;
  mixed    the cow's triangles and 256 spheres above them in one bvh_node, and a loose sphere light (k_paths_g).
S1 is S0 with every small sphere (radius < 10), the moving ones as well, displaced by a seeded uniform offset in
[-0.5, 0.5]^2 in x and z.

Every round:
  (i)  scene A (compiled with S0) is updated to S1 from a device tensor: the device time of the update's kernels (HIP
       events) and the host wall time of the call; scene B is compiled fresh with S1 and uploaded: host wall time of
       rt_graph_compile + the upload (the Python calls that rebuild the graph are timed apart and not counted).
  (ii) A and B render W x H x spp: segments per millisecond of device time; the frames must be equal bit for bit.
A goes back to S0 before the next round, so every timed update is the same one.  --warmup rounds, then --runs timed
ones; medians, minima and maxima, the ratios of the medians, and whether a difference exceeds the rounds' spread.

Prints one JSON line (kept as profiles/sphere_update_time.json).

  python tools/sphere_update_time.py [--scenes spheres,mixed] [--shape 1920x1080x16] [--runs 15] [--warmup 3]
"""
import numpy as np

import _update_timing as ut


def quant(a):
    """Multiples of 2^-20: a moving sphere's center1 - center0 is then the same double in every compile."""
    return np.round(np.asarray(a, np.float64) * 2.0 ** 20) / 2.0 ** 20


def spheres_scene(art):
    """(S0, graph, camera arguments): scene 1's spheres with seeded materials."""
    one = art.scene_manager().build("1")
    s0 = quant(art.scene_spheres(one))
    rng = np.random.default_rng(1)
    kind = rng.integers(0, 64, len(s0))
    colour = rng.uniform(0.1, 0.9, (64, 3))

    def graph(s):
        art.reset_scene_rng()
        # a palette of 64 materials (48 lambertian, 12 metal, 4 dielectric) and the ground's: the image's shading table
        # holds them all, so the scene runs k_paths as the builtin one does
        palette = [art.lambertian(tuple(colour[m])) if m < 48 else art.metal(tuple(colour[m]), 0.2) if m < 60 else art.dielectric(1.5) for m in range(64)]
        ground = art.lambertian((0.5, 0.5, 0.5))
        objs = []
        for k, (x, y, z, r) in enumerate(s):
            mat = ground if r > 10.0 else palette[kind[k]]
            if r < 0.5 and k % 8 == 3:
                objs.append(art.moving_sphere((x, y, z), (x, y + 0.25, z), 0.0, 1.0, r, mat))
            else:
                objs.append(art.sphere((x, y, z), r, mat))
        w = art.hittable_list()
        w.add(art.bvh_node(objs))
        return w
    return s0, graph, (one.lookfrom, one.lookat, one.vfov)


def mixed_scene(art):
    tris = art.scene_triangles(art.scene_manager().build("cow"))
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    c, ext = 0.5 * (lo + hi), float((hi - lo).max())
    rng = np.random.default_rng(2)
    s0 = np.zeros((257, 4))
    g = np.linspace(-1.0, 1.0, 16)
    for k in range(256):
        s0[k] = (c[0] + ext * g[k % 16], hi[1] + rng.uniform(0.1, 0.4) * ext, c[2] + ext * g[k // 16], rng.uniform(0.01, 0.03) * ext)
    s0[256] = (c[0], hi[1] + 3.0 * ext, c[2], 0.5 * ext)
    s0 = quant(s0)

    def graph(s):
        art.reset_scene_rng()
        mat, shiny, light = art.lambertian((0.7, 0.6, 0.5)), art.metal((0.8, 0.8, 0.8), 0.1), art.diffuse_light((4.0, 4.0, 4.0))
        objs = [art.triangle(t[0], t[1], t[2], mat) for t in tris]
        objs += [art.sphere(tuple(s[k, :3]), float(s[k, 3]), shiny if k % 2 else mat) for k in range(256)]
        w = art.hittable_list()
        w.add(art.bvh_node(objs))
        w.add(art.sphere(tuple(s[256, :3]), float(s[256, 3]), light))
        return w
    return s0, graph, ((c[0] + 0.4 * ext, c[1] + 1.2 * ext, c[2] + 2.4 * ext), tuple(c), 40.0)


def main():
    art, torch, args, (W, H, k), result = ut.start("sphere_update_time", "scenes", "spheres,mixed", 15, {
        "update_device_ms": "HIP events around the update's kernels", "update_wall_ms": "host wall time of update_spheres(timing=True)"})
    for name in args.scenes.split(","):
        s0, graph, (lookfrom, lookat, vfov) = {"spheres": spheres_scene, "mixed": mixed_scene}[name](art)
        rng = np.random.default_rng(3)
        s1 = np.array(s0)
        small = s0[:, 3] < 10.0
        s1[small, 0] += rng.uniform(-0.5, 0.5, int(small.sum()))
        s1[small, 2] += rng.uniform(-0.5, 0.5, int(small.sum()))
        s1 = quant(s1)
        render = ut.renderer(art, art.camera(lookfrom, lookat, (0, 1, 0), vfov, W / H, 0.0, 10.0, 0.0, 1.0), (W, H, k))
        a = ut.compiled(art, graph(s0))
        nodes, refs = art.scene_bvh(a)
        has_image = art.scene_lds_image(a) is not None
        t_s0, t_s1 = torch.from_numpy(np.array(s0)).cuda(), torch.from_numpy(s1).cuda()
        torch.cuda.synchronize()
        equal, kernel = True, None
        ms, rate = {}, {}
        for r in range(args.warmup + args.runs):
            m, b, w = ut.update_then_fresh(art, lambda: art.update_spheres(a, t_s1, timing=True), lambda: graph(s1))
            img_a, rate_a, st = render(a)
            img_b, rate_b, _ = render(b)
            art.update_spheres(a, t_s0)  # back to S0: the next round's update is this round's
            torch.cuda.synchronize()
            equal = equal and bool((img_a == img_b).all())
            kernel = [st["kernel_features"], st["kernel_textures"], st["kernel_lds_mode"], st["extend_variant"]]
            del b, w
            ut.record(args, r, ms, m, rate, {"refit_moved": rate_a, "fresh_moved": rate_b})
        entry = {"spheres": int(len(s0)), "bvh_nodes": int(len(nodes)), "leaf_slots": int(len(refs)), "lds_image": has_image, "kernel": kernel,
                 "frames_equal_bit_for_bit": equal}
        result["scenes"][name] = ut.finish(entry, ms, rate, [("refit_moved", "fresh_moved", "refit", "")])
        del a
        torch.cuda.empty_cache()
    ut.report(result)


if __name__ == "__main__":
    main()
