"""Updates of different kinds on one scene.  rt_scene_update_triangles and rt_scene_update_spheres share what a scene's
first geometry update makes (the slot boxes, the pad flags, the level table), and all four update calls run one host
path; a scene that holds triangles and spheres in one bvh_node takes three updates -- triangles, spheres, textures plus
materials -- in every order and must then give, bit for bit, what a scene compiled fresh from the new values gives: a
32 x 32 x 2 frame, 256 queries, the four getters; and every box of its refitted tree is the specified one.

`grid`: an 8 x 8 height field (128 triangles) and 16 spheres in one bvh_node, a loose sphere light.  `capsule`: the
capsule's 10 200 triangles and 3 spheres in one bvh_node (more than 8192 references: an F_LEAF2 kernel on a padded copy
of the references, whose pad slots read as sphere 0 -- k_update_spheres skips them by their flag, k_update_tris by their
type), the same light.  Materials: two lambertians over one shared solid colour, a third over its own, a metal, a
dielectric, the light."""
import functools
import itertools

import numpy as np
import pytest

import another_raytracer_amd as art
from tests.update_common import (ASSETS, F_LEAF2, F32, SKY, bits, conservative_box_np, covered_slots, grid_triangles, kernel_of, quant, render,
                                 same_queries, same_render, v3)

pytestmark = pytest.mark.gpu

SIZE = (32, 32, 2)
NRAYS = 256
METAL_ID, GLASS_ID = 3, 4


def box_of(p):
    lo, hi = p.reshape(-1, 3).min(0), p.reshape(-1, 3).max(0)
    return lo, hi, 0.5 * (lo + hi), float((hi - lo).max())


def build(p, s, m, t):
    """The world of triangles p (n, 3, 3), spheres s (k + 1, 4: k in the bvh_node, then the loose light), material rows m
    (6, 5) and texture rows t (3, 4) in the getters' layouts.  The same call sequence for every value, so ids agree."""
    art.reset_scene_rng()
    shared, own, emit = art.solid_color(*v3(t[0, :3])), art.solid_color(*v3(t[1, :3])), art.solid_color(*v3(t[2, :3]))
    mats = [art.lambertian(shared), art.lambertian(shared), art.lambertian(own), art.metal(v3(m[METAL_ID, :3]), float(m[METAL_ID, 3])),
            art.dielectric(float(m[GLASS_ID, 4]))]
    light = art.diffuse_light(emit)
    assert [x.id for x in (shared, own, emit)] == [0, 1, 2] and [x.id for x in mats + [light]] == list(range(6))
    objs = [art.sphere(v3(s[k, :3]), float(s[k, 3]), mats[2 + k % 3]) for k in range(len(s) - 1)]  # spheres first: reference 0 is a sphere
    objs += [art.triangle(q[0], q[1], q[2], mats[i % 3]) for i, q in enumerate(p)]
    w = art.hittable_list()
    w.add(art.bvh_node(objs))
    w.add(art.sphere(v3(s[-1, :3]), float(s[-1, 3]), light))
    return art.hittable_list(native=art.compile_world(w, 0))


M0 = np.zeros((6, 5))
M0[METAL_ID, :4], M0[GLASS_ID, 4] = (0.7, 0.6, 0.5, 0.125), 1.5
T0 = np.array([[0.8, 0.3, 0.3, 0.0], [0.3, 0.8, 0.3, 0.0], [4.0, 4.0, 4.0, 0.0]])
M1 = np.zeros((6, 5))
M1[METAL_ID, :4], M1[GLASS_ID, 4] = (0.25, 0.5, 0.875, 0.375), 1.75
T1 = np.array([[0.125, 0.5, 0.75, 0.0], [0.875, 0.625, 0.25, 0.0], [6.0, 5.0, 3.0, 0.0]])


@functools.lru_cache(maxsize=None)
def values(name):
    """(P0, S0, P1, S1) of a world, read-only.  P1: every vertex moved, seeded, by up to a twentieth of the mesh's extent
    per axis, and the mesh stretched 1.25 x in x about its centre; S1: centres moved by up to a radius per axis, radii
    scaled by [0.7, 1.3]."""
    rng = np.random.default_rng(61)
    if name == "grid":
        p0 = grid_triangles(8)
        s0 = np.array([(-2.25 + 1.5 * (k % 4) + rng.uniform(-0.2, 0.2), rng.uniform(2.2, 3.0), -2.25 + 1.5 * (k // 4) + rng.uniform(-0.2, 0.2),
                        rng.uniform(0.2, 0.35)) for k in range(16)] + [(0.0, 9.0, 0.0, 1.5)])
    else:
        p0 = art.scene_triangles(art.scene_manager(ASSETS).build("9"))
        lo, hi, c, ext = box_of(p0)
        s0 = np.array([[c[0], hi[1] + 0.8 * ext, c[2], 0.3 * ext], [lo[0] - ext, c[1], c[2], 0.4 * ext], [hi[0] + 0.8 * ext, c[1], c[2], 0.3 * ext],
                       [c[0], hi[1] + 3.0 * ext, c[2], 0.5 * ext]])
    lo, hi, c, ext = box_of(p0)
    p1 = p0 + rng.uniform(-0.05, 0.05, p0.shape) * ext
    p1[..., 0] = c[0] + 1.25 * (p1[..., 0] - c[0])
    s0 = quant(s0)
    s1 = np.array(s0)
    s1[:, :3] += rng.uniform(-1.0, 1.0, (len(s0), 3)) * (0.2 if name == "capsule" else 1.0) * s0[:, 3:4]  # (capsule: stay clear of the mesh)
    s1[:, 3] *= rng.uniform(0.7, 1.3, len(s0))
    out = (np.ascontiguousarray(p0), s0, np.ascontiguousarray(p1), quant(s1))
    for x in out:
        x.setflags(write=False)
    return out


def frame_camera(name):
    lo, hi, c, ext = box_of(values(name)[2])
    return art.camera((c[0] + 0.4 * ext, c[1] + 0.9 * ext, c[2] + 2.6 * ext), tuple(c), (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)


def query_rays(name):
    lo, hi, c, ext = box_of(values(name)[2])
    rng = np.random.default_rng(11)
    o = rng.normal(size=(NRAYS, 3))
    o = c + 3.0 * ext * o / np.linalg.norm(o, axis=1, keepdims=True)
    target = rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext + [0.0, ext, 0.0], (NRAYS, 3))  # the spheres sit above the mesh
    rays = np.zeros((NRAYS, 7))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, target - o, rng.uniform(0, 1, NRAYS)
    return rays


@functools.lru_cache(maxsize=None)
def fresh(name):
    """The world compiled from V1 with its frame and what its getters give: computed once, read by every order."""
    p0, s0, p1, s1 = values(name)
    b = build(p1, s1, M1, T1)
    return b, render(b, frame_camera(name), SKY, SIZE), (art.scene_triangles(b), art.scene_spheres(b), art.scene_materials(b), art.scene_textures(b))


def the_boxes_are_the_specified_ones(nodes, refs, tris, spheres):
    """tests/test_gpu_update_spheres.py and test_gpu_update_triangles.py test_the_refitted_boxes_are_the_specified_ones' check,
    for leaves that hold either kind: a leaf's box is refit.h's conservative box of its primitives' f64 boxes, an inner
    child's the union of that node's live boxes, an empty child's the empty box."""
    planes = lambda n, c: (np.array([nodes["lox"][n, c], nodes["loy"][n, c], nodes["loz"][n, c]]),  # noqa: E731
                           np.array([nodes["hix"][n, c], nodes["hiy"][n, c], nodes["hiz"][n, c]]))
    prim_lo = [spheres[:, :3] - spheres[:, 3:4], tris.min(1)]  # by reference type: 0 a sphere, 1 a triangle
    prim_hi = [spheres[:, :3] + spheres[:, 3:4], tris.max(1)]
    leaves = inner = both = 0
    for n in range(len(nodes)):
        for c in range(4):
            code = int(nodes["child"][n, c])
            lo, hi = planes(n, c)
            if code == -1:
                assert (lo == np.finfo(F32).max).all() and (hi == -np.finfo(F32).max).all()
            elif code < 0:
                first, count = ~code & 0xFFFFFF, (~code >> 24) & 0x7F
                r = refs[first:first + count]
                ty, idx = r >> 30, r & (2 ** 30 - 1)
                assert (ty <= 1).all()
                wl, wh = conservative_box_np(np.min([prim_lo[t][i] for t, i in zip(ty, idx)], 0), np.max([prim_hi[t][i] for t, i in zip(ty, idx)], 0))
                assert (lo.view(np.int32) == wl.view(np.int32)).all() and (hi.view(np.int32) == wh.view(np.int32)).all(), (n, c)
                leaves += 1
                both += len(set(ty.tolist())) == 2
            else:
                assert code > n
                live = nodes["child"][code] != -1
                wl = np.array([nodes[f][code][live].min() for f in ("lox", "loy", "loz")])
                wh = np.array([nodes[f][code][live].max() for f in ("hix", "hiy", "hiz")])
                assert (lo == wl).all() and (hi == wh).all(), (n, c)
                inner += 1
    assert leaves > len(tris) // 8 and inner == len(nodes) - 1  # every node but the root is some node's child
    return both


KINDS = ("triangles", "spheres", "appearance")
ORDERS = [("grid", order) for order in itertools.permutations(KINDS)]
# the pair-aligned scene: whichever geometry kind comes first makes the slot boxes and the pad flags the other one then uses
ORDERS += [("capsule", ("triangles", "spheres", "appearance")), ("capsule", ("spheres", "appearance", "triangles"))]


@pytest.mark.parametrize("name,order", ORDERS, ids=[f"{n}-{'-'.join(k[0] for k in o)}" for n, o in ORDERS])
def test_updates_of_every_kind_in_any_order_equal_the_fresh_compile(gpu, name, order):
    p0, s0, p1, s1 = values(name)
    a, cam = build(p0, s0, M0, T0), frame_camera(name)
    before = render(a, cam, SKY, SIZE)
    assert bool(before[2]["kernel_features"] & F_LEAF2) == (name == "capsule")
    nodes0, refs0 = art.scene_bvh(a)
    pads = ~covered_slots(nodes0, len(refs0))
    if name == "capsule":
        assert pads.sum() > 100 and (refs0[pads] == 0).sum() > 100  # pad slots exist, and read as sphere 0
    assert (bits(art.scene_spheres(a)) == bits(s0)).all() and (bits(art.scene_triangles(a)) == bits(p0)).all()
    steps = {"triangles": lambda: art.update_triangles(a, p1), "spheres": lambda: art.update_spheres(a, s1),
             "appearance": lambda: (art.update_textures(a, T1), art.update_materials(a, M1))}
    for kind in order:
        steps[kind]()
    b, frame_b, (pb, sb, (mb, mdb), (tb, tdb)) = fresh(name)
    # the frame
    ra = render(a, cam, SKY, SIZE)
    assert same_render(ra, frame_b), (int((ra[0] != frame_b[0]).sum()), ra[2]["segments"], frame_b[2]["segments"])
    assert not same_render(ra, before) and ra[0].max() > 0 and kernel_of(ra[2]) == kernel_of(before[2])
    # closest hits and occlusion
    hits = same_queries(a, b, query_rays(name))
    assert np.isfinite(hits[:, 0]).any() and (hits[:, 10] >= 2 ** 30).any() and ((hits[:, 10] >= 0) & (hits[:, 10] < 2 ** 30)).any()  # both kinds are hit
    # the getters
    (ma, mda), (ta, tda) = art.scene_materials(a), art.scene_textures(a)
    assert (bits(art.scene_triangles(a)) == bits(pb)).all() and (bits(pb) == bits(p1)).all()
    assert (bits(art.scene_spheres(a)) == bits(sb)).all() and (bits(sb) == bits(s1)).all()
    assert (bits(ma) == bits(mb)).all() and (mda == mdb).all() and (bits(ma[METAL_ID:GLASS_ID + 1]) == bits(M1[METAL_ID:GLASS_ID + 1])).all()
    assert (bits(ta) == bits(tb)).all() and (tda == tdb).all() and (bits(ta) == bits(T1)).all()
    # the tree: the topology and the references stay, every box is the specified one
    nodes, refs = art.scene_bvh(a)
    assert len(nodes) == len(nodes0) and (nodes["child"] == nodes0["child"]).all() and (nodes["pad"] == nodes0["pad"]).all() and (refs == refs0).all()
    changed = sum(int((nodes[f] != nodes0[f]).sum()) for f in ("lox", "hix", "loy", "hiy", "loz", "hiz"))
    assert changed > len(nodes)  # the updates did move the boxes
    the_boxes_are_the_specified_ones(nodes, refs, p1, s1)
