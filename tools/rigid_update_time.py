#!/usr/bin/env python3
"""Times rt_scene_update_objects, and rt_scene_update_rects + rt_scene_update_boxes, against what the library offered before
them -- a fresh compile and upload of the same values -- and compares the render rates of the updated and the freshly
compiled scene, in one process on one GPU.  The scenes are the builtin rigid ones, rebuilt here call for call from the
package's constructors (checked against the builtin scene's getters bit for bit) so that a fresh compile can take new values:
  6  the Cornell box: six rects in one BVH, two translate(rotate_y(box));
  7  the Cornell smoke box: the same with a constant_medium over each box chain;
  8  the Next-Week final scene: 400 boxes, a rect light and four spheres in one BVH, two media over spheres, two loose
     spheres, and translate(rotate_y(bvh_node of 1000 spheres)).
V1, seeded: every angle + 20 degrees, every offset moved by (30, 10, -25), every density doubled (objects); every rect's
a0, a1, b0, b1 and k moved by up to 5, every box's min lowered by up to 3 and max raised by up to 6 per axis (rects + boxes).

Two measurements per scene, each over --warmup + --runs rounds.  Every round:
  (i)  scene A (compiled with V0) is updated to V1 from device tensors: the device time of the calls' kernels (HIP events,
       summed) and the host wall time of the calls; scene B is compiled fresh with V1 and uploaded: host wall time of
       rt_graph_compile + the upload (the Python calls that rebuild the graph are timed apart and not counted).
  (ii) A and B render W x H x spp, A first in even rounds and B first in odd ones: segments per millisecond of device
       time; whether the frames are equal bit for bit is recorded per round (warm-up rounds included).
A goes back to V0 before the next round, so every timed update is the same one.  An objects update keeps the tree the fresh
compile builds: its render rate should equal the fresh compile's within the rounds' spread.  A rects + boxes update keeps
the V0 topology with refitted boxes: the ratio is reported as measured.

Prints one JSON line (kept as profiles/rigid_update_time.json); a progress line per measurement goes to stderr.

  python tools/rigid_update_time.py [--scenes 6,7,8] [--shape 1920x1080x16] [--runs 15] [--warmup 3]
"""
import ctypes
import os
import sys

import numpy as np

import _update_timing as ut

ASSETS = os.path.join(ut.ROOT, "assets")
# the scenes' own angles (degrees), offsets and densities, in world order (scene_manager.cpp:106-234)
NATURAL = {"6": dict(ANG=[15.0, -18.0], OFF=[(265.0, 0.0, 295.0), (130.0, 0.0, 65.0)], DENS=[]),
           "7": dict(ANG=[15.0, -18.0], OFF=[(265.0, 0.0, 295.0), (130.0, 0.0, 65.0)], DENS=[0.01, 0.01]),
           "8": dict(ANG=[15.0], OFF=[(-100.0, 270.0, 395.0)], DENS=[0.2, 0.0001])}


def v3(x):
    return tuple(float(t) for t in x)


def cornell(art, smoke, v):
    """scene_manager.cpp:106-169 with the rects' rows, the boxes' rows, the angles, offsets and densities from v."""
    art.reset_scene_rng()
    red, white, green = art.lambertian((.65, .05, .05)), art.lambertian((.73, .73, .73)), art.lambertian((.12, .45, .15))
    lv = 7.0 if smoke else 15.0
    light = art.diffuse_light(art.solid_color(lv, lv, lv))
    R, B = v["R"], v["B"]
    w = art.hittable_list()
    w.add(art.yz_rect(*R[0], green))
    w.add(art.yz_rect(*R[1], red))
    w.add(art.xz_rect(*R[2], light))
    w.add(art.xz_rect(*R[3], white))
    w.add(art.xz_rect(*R[4], white))
    w.add(art.xy_rect(*R[5], white))
    chains = [art.translate(art.rotate_y(art.box(v3(B[k, :3]), v3(B[k, 3:]), white), float(v["ANG"][k])), v3(v["OFF"][k])) for k in range(2)]
    if not smoke:
        w.add(chains[0])
        w.add(chains[1])
    else:
        w.add(art.constant_medium(chains[0], float(v["DENS"][0]), (0.0, 0.0, 0.0)))
        w.add(art.constant_medium(chains[1], float(v["DENS"][1]), (1.0, 1.0, 1.0)))
    return w


def final(art, v):
    """scene_manager.cpp:171-234, every draw from the shared generator in the reference's order (the box heights are drawn
    even when v holds other ones, so the perlin table and the 1000 spheres stay what they are)."""
    art.reset_scene_rng()
    R, B = v["R"], v["B"]
    ground = art.lambertian((0.48, 0.83, 0.53))
    boxes1 = []
    for i in range(20):
        for j in range(20):
            art.random_double(1, 101)  # the box's height y1; V0's row is (x0, 0, z0, x0 + 100, y1, z0 + 100), x0 = -1000 + 100 i, z0 = -1000 + 100 j
            row = B[len(boxes1)]
            boxes1.append(art.box(v3(row[:3]), v3(row[3:]), ground))
    w = art.hittable_list()
    w.add(art.bvh_node(boxes1))
    w.add(art.xz_rect(*R[0], art.diffuse_light(art.solid_color(7.0, 7.0, 7.0))))
    w.add(art.moving_sphere((400, 400, 200), (430, 400, 200), 0, 1, 50, art.lambertian((0.7, 0.3, 0.1))))
    w.add(art.sphere((260, 150, 45), 50, art.dielectric(1.5)))
    w.add(art.sphere((0, 150, 145), 50, art.metal((0.8, 0.8, 0.9), 1.0)))
    boundary = art.sphere((360, 150, 145), 70, art.dielectric(1.5))
    w.add(boundary)
    w.add(art.constant_medium(boundary, float(v["DENS"][0]), (0.2, 0.4, 0.9)))
    w.add(art.constant_medium(art.sphere((0, 0, 0), 5000, art.dielectric(1.5)), float(v["DENS"][1]), (1.0, 1.0, 1.0)))
    w.add(art.sphere((400, 200, 400), 100, art.lambertian(art.image_texture(os.path.join(ASSETS, "earthmap.rgb")))))
    w.add(art.sphere((220, 280, 300), 80, art.lambertian(art.noise_texture(0.1))))
    white = art.lambertian((.73, .73, .73))
    boxes2 = []
    for _ in range(1000):  # vec3::random's three draws land in z, y, x: the reference's compiler evaluates the arguments right to left
        z, y, x = art.random_double(0, 165), art.random_double(0, 165), art.random_double(0, 165)
        boxes2.append(art.sphere((x, y, z), 10, white))
    w.add(art.translate(art.rotate_y(art.bvh_node(boxes2), float(v["ANG"][0])), v3(v["OFF"][0])))
    return w


def graph_of(art, name, v):
    return final(art, v) if name == "8" else cornell(art, name == "7", v)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_scene(art, a, b):
    """Every getter of the worlds a and b agrees bit for bit."""
    same = (bits(art.scene_spheres(a)) == bits(art.scene_spheres(b))).all()
    for get in (art.scene_rects, art.scene_boxes, art.scene_objects, art.scene_materials, art.scene_textures):
        (va, da), (vb, db) = get(a), get(b)
        same = same and va.shape == vb.shape and (bits(va) == bits(vb)).all() and (da == db).all()
    return bool(same)


def new_values(name, R0, B0, seed=4):
    rng = np.random.default_rng(seed)
    nat = NATURAL[name]
    objects = dict(ANG=[a + 20.0 for a in nat["ANG"]], OFF=[(x + 30.0, y + 10.0, z - 25.0) for x, y, z in nat["OFF"]], DENS=[2.0 * d for d in nat["DENS"]])
    R1 = R0 + rng.uniform(-5.0, 5.0, R0.shape)
    B1 = np.array(B0)
    B1[:, :3] -= rng.uniform(0.0, 3.0, (len(B0), 3))
    B1[:, 3:] += rng.uniform(0.0, 6.0, (len(B0), 3))
    return objects, R1, B1


def main():
    art, torch, args, (W, H, k), result = ut.start("rigid_update_time", "scenes", "6,7,8", 15, {
        "update_device_ms": "HIP events around each call's kernels: update_objects, or update_rects + update_boxes",
        "update_wall_ms": "host wall time of the call(s) (timing=True: each waits)"})
    for name in args.scenes.split(","):
        builtin = art.scene_manager(ASSETS).build(name)
        (R0, _), (B0, _) = art.scene_rects(builtin), art.scene_boxes(builtin)
        v0 = dict(NATURAL[name], R=R0, B=B0)
        a = ut.compiled(art, graph_of(art, name, v0))
        assert same_scene(art, a, builtin.objects), f"scene {name}: the rebuilt graph is not the builtin scene"
        objects1, R1, B1 = new_values(name, R0, B0)
        measured = {"objects": (dict(objects1, R=R0, B=B0), ("P",)), "rects_boxes": (dict(NATURAL[name], R=R1, B=B1), ("R", "B"))}
        render = ut.renderer(art, art.camera(builtin.lookfrom, builtin.lookat, (0, 1, 0), builtin.vfov, W / H, builtin.aperture, 10.0, 0.0, 1.0), (W, H, k))
        (P0, Pd) = art.scene_objects(a)
        img_v0 = render(a)[0]
        nodes = ctypes.c_int64()
        refs = ctypes.c_int64()
        art._lib.check(art.lib.rt_scene_bvh_get(a._native, None, 0, None, 0, ctypes.byref(nodes), ctypes.byref(refs)), "counts")
        entry = {"rects": int(len(R0)), "boxes": int(len(B0)), "object_records": int(len(P0)), "translates": int((Pd[:, 0] == art.OBJ_TRANSLATE).sum()),
                 "rotates": int((Pd[:, 0] == art.OBJ_ROTATE_Y).sum()), "media": int((Pd[:, 0] == art.OBJ_MEDIUM).sum()), "nodes": nodes.value, "slots": refs.value}
        for what, (v1, kinds) in measured.items():
            first = ut.compiled(art, graph_of(art, name, v1), upload=False)
            P1 = art.scene_objects(first)[0]
            del first
            dev = {key: (torch.from_numpy(np.array(x0)).cuda(), torch.from_numpy(np.array(x1)).cuda()) for key, (x0, x1) in (("P", (P0, P1)), ("R", (R0, R1)), ("B", (B0, B1)))}
            call = {"P": art.update_objects, "R": art.update_rects, "B": art.update_boxes}
            torch.cuda.synchronize()
            kernel, equal = None, []
            ms, rate = {}, {}
            for r in range(args.warmup + args.runs):
                m, b, w = ut.update_then_fresh(art, lambda: sum(call[key](a, dev[key][1], timing=True) for key in kinds), lambda: graph_of(art, name, v1))
                # the two renders alternate their order from round to round: whichever runs first after the compile's idle
                # gap measured 1-2 % slower, on either scene
                if r % 2 == 0:
                    (img_a, rate_a, st), (img_b, rate_b, _) = render(a), render(b)
                else:
                    (img_b, rate_b, _), (img_a, rate_a, st) = render(b), render(a)
                equal.append(bool((img_a == img_b).all()))
                assert (img_a != img_v0).any(), f"scene {name}, {what}: the update is not visible"
                if r == 0:
                    assert same_scene(art, a, b), f"scene {name}, {what}: the updated scene's getters differ from the fresh compile's"
                for key in kinds:  # back to V0: the next round's update is this round's
                    call[key](a, dev[key][0])
                torch.cuda.synchronize()
                kernel = [st["kernel_features"], st["kernel_textures"], st["kernel_lds_mode"], st["extend_variant"]]
                del b, w
                ut.record(args, r, ms, m, rate, {"updated": rate_a, "fresh": rate_b})
            print(f"scene {name}, {what}: {sum(equal)} of {len(equal)} rounds with equal frames", file=sys.stderr, flush=True)
            entry[what] = ut.finish({"kernel": kernel, "frames_equal_bit_for_bit": all(equal), "rounds_with_equal_frames": sum(equal), "rounds": len(equal)}, ms, rate,
                                    [("updated", "fresh", "updated", "")])
        result["scenes"][name] = entry
        del a
        torch.cuda.empty_cache()
    ut.report(result)


if __name__ == "__main__":
    main()
