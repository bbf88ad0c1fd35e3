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
import numpy as np

import _update_timing as ut
from sphere_update_time import mixed_scene, spheres_scene

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
    art, torch, args, (W, H, k), result = ut.start("material_update_time", "scenes", "spheres,mixed", 15, {
        "update_device_ms": "HIP events around each call's kernels, update_materials + update_textures",
        "update_wall_ms": "host wall time of the two calls (timing=True: each waits)"})
    for name in args.scenes.split(","):
        s0, graph0, (lookfrom, lookat, vfov) = {"spheres": spheres_scene, "mixed": mixed_scene}[name](art)
        a = ut.compiled(art, graph0(s0))
        (M0, Md), (T0, Td) = art.scene_materials(a), art.scene_textures(a)
        M1, T1 = new_values(M0, Md, T0, Td)
        # the same graph function over the package with V1 in its constructors
        _, graph1, _ = {"spheres": spheres_scene, "mixed": mixed_scene}[name](WithValues(art, M1, T1))
        render = ut.renderer(art, art.camera(lookfrom, lookat, (0, 1, 0), vfov, W / H, 0.0, 10.0, 0.0, 1.0), (W, H, k))
        has_image = art.scene_lds_image(a) is not None
        img_v0 = render(a)[0]
        dev = [torch.from_numpy(np.array(x)).cuda() for x in (M0, T0, M1, T1)]
        torch.cuda.synchronize()
        kernel = None
        ms, rate = {}, {}
        for r in range(args.warmup + args.runs):
            m, b, w = ut.update_then_fresh(art, lambda: art.update_materials(a, dev[2], timing=True) + art.update_textures(a, dev[3], timing=True),
                                           lambda: graph1(s0))
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
            ut.record(args, r, ms, m, rate, {"updated": rate_a, "fresh": rate_b})
        entry = {"materials": int(len(M0)), "textures": int(len(T0)), "metals": int((Md[:, 0] == METAL).sum()), "dielectrics": int((Md[:, 0] == DIELECTRIC).sum()),
                 "solid_colours": int((Td[:, 0] == SOLID).sum()), "lds_image": has_image, "kernel": kernel, "frames_equal_bit_for_bit": True}
        result["scenes"][name] = ut.finish(entry, ms, rate, [("updated", "fresh", "updated", "")])
        del a
        torch.cuda.empty_cache()
    ut.report(result)


if __name__ == "__main__":
    main()
