"""rt_scene_update_rects, rt_scene_update_boxes and rt_scene_update_objects on the device.  A scene compiled from values V0
and updated to V1 must give, bit for bit, what a scene compiled fresh from V1 gives: a 32 x 32 x 2 frame (RGB8, f64 sums,
segment count), 256 closest-hit records and any-hit bytes, the getters; the kernel it runs must not change; and every box
of a refitted tree is the specified one.

`room`: five wall rects and a light rect in a row (world merging makes them one BVH of rects), two
translate(rotate_y(box)), a constant_medium over a third such chain and a constant_medium over a sphere.  `field`: one
bvh_node of 16 boxes, 8 rects (a floor among them) and 8 spheres, and an xz_rect light beside it in the world list.
`loose`: an xz_rect and a translate(box) only -- no BVH, no leaf slots, nothing to refit.  Every value is seeded random
and unquantised.

Closest hits are tree-independent only up to exact-t ties, and the refitted and the fresh tree differ: every test
asserts that within one BVH no two rect planes or box faces share a coordinate on an axis."""
import functools

import numpy as np
import pytest

import another_raytracer_amd as art
from tests.update_common import ASSETS, F32, SKY, bits, conservative_box_np, kernel_of, render, same_queries, same_render, v3

pytestmark = pytest.mark.gpu

SIZE = (32, 32, 2)
NRAYS = 256
SEED = 5  # update_common.engine_for's
PRIM, BVH, TRANSLATE, ROTATE_Y, MEDIUM = range(5)
RECT_CLASS = {0: art.xy_rect, 1: art.xz_rect, 2: art.yz_rect}
METAL_ID, GLASS_ID = 3, 4


def frozen(**arrays):
    for a in arrays.values():
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------ the worlds' values
@functools.lru_cache(maxsize=None)
def values(name, which):
    """The world's values V0 (which = 0) or V1 (1), read-only: R rect rows, AX their axes, B box rows, ANG angles in
    degrees, OFF offsets, DENS densities, S sphere rows, M material rows (scene_materials' layout).  What a world does not
    hold is empty."""
    rng = np.random.default_rng((17, 29)[which] + sum(map(ord, name)))
    u = lambda lo, hi, *shape: rng.uniform(lo, hi, shape)  # noqa: E731
    none = dict(R=np.zeros((0, 5)), AX=np.zeros(0, int), B=np.zeros((0, 6)), ANG=np.zeros(0), OFF=np.zeros((0, 3)), DENS=np.zeros(0), S=np.zeros((0, 4)),
                M=np.zeros((6, 5)))
    none["M"][METAL_ID, :4], none["M"][GLASS_ID, 4] = ((0.7, 0.6, 0.5, 0.125), (0.25, 0.5, 0.875, 0.375))[which], (1.5, 1.75)[which]
    if name == "room":  # a 10-unit Cornell box, open toward -z
        r = np.array([[0, 10, 0, 10, 10], [0, 10, 0, 10, 0], [3.5, 6.5, 3.5, 6.5, 9.2], [0, 10, 0, 10, 0], [0, 10, 0, 10, 10], [0, 10, 0, 10, 10]], float)
        b = np.array([[0, 0, 0, 3, 6, 3], [0, 0, 0, 3, 3, 3], [0, 0, 0, 2, 2, 2]], float)
        b[:, :3] += u(-0.2, 0.2, 3, 3)
        b[:, 3:] += u(-0.4, 0.4, 3, 3)
        return frozen(**{**none, "R": r + u(-0.3, 0.3, 6, 5), "AX": np.array([2, 2, 1, 1, 1, 0]), "B": b, "ANG": np.array([15.0, -18.0, 30.0]) + u(-10, 10, 3),
                         "OFF": np.array([[4.8, 0, 5.3], [2.3, 0, 1.2], [6.5, 0.5, 1.0]]) + u(-0.5, 0.5, 3, 3), "DENS": np.array([0.5, 0.3]) * u(0.5, 2.0, 2)})
    if name == "field":  # a 4 x 4 grid of cells of pitch 2 over [-4, 4]^2
        cx, cz = (-3.0 + 2.0 * (np.arange(16) % 4)), (-3.0 + 2.0 * (np.arange(16) // 4))
        # Kinds share a leaf where the builder gains nothing by parting them -- two primitives with nearly one bounding box:
        # an even cell holds a cube with a sphere that just pokes through its faces, cells 1, 7 and 13 a flat box with a
        # lid through it that juts out all round.  The other odd cells hold boxes of random height with a panel beside them.
        h = u(0.5, 1.5, 16)
        h[::2], h[[1, 7, 13]] = 1.2, 0.3
        b = np.stack([cx - 0.6, np.zeros(16), cz - 0.6, cx + 0.6, h, cz + 0.6], 1) + u(-0.05, 0.05, 16, 6)
        s = np.stack([cx[::2] + u(-0.05, 0.05, 8), 0.6 + u(-0.05, 0.05, 8), cz[::2] + u(-0.05, 0.05, 8), u(0.62, 0.7, 8)], 1)
        ax = np.array([1, 1, 2, 0, 1, 2, 0, 1, 1])  # the floor, seven lids and panels at the odd boxes, the light
        r = np.zeros((9, 5))
        r[0] = (-5, 5, -5, 5, -0.05)
        for k in range(1, 8):
            c = 2 * k - 1  # an odd cell
            if ax[k] == 2:    # yz: a panel beside the box
                r[k] = (0.1, 1.2, cz[c] - 0.5, cz[c] + 0.5, cx[c] + 0.85)
            elif ax[k] == 0:  # xy: a panel behind it
                r[k] = (cx[c] - 0.5, cx[c] + 0.5, 0.1, 1.2, cz[c] + 0.85)
            else:             # xz: a lid through it
                r[k] = (cx[c] - 0.7, cx[c] + 0.7, cz[c] - 0.7, cz[c] + 0.7, 0.15)
        r[8] = (-2, 2, -2, 2, 3.0)  # low enough for the floor to hold half the BVH's box area: the builder hoists it
        return frozen(**{**none, "R": r + u(-0.05, 0.05, 9, 5), "AX": ax, "B": b, "S": s})
    assert name == "loose"
    return frozen(**{**none, "R": np.array([[-3, 3, -3, 3, 0.0]]) + u(-0.3, 0.3, 1, 5), "AX": np.array([1]),
                     "B": np.array([[-1, 0, -1, 1, 1.5, 1.0]]) + u(-0.3, 0.3, 1, 6), "OFF": np.array([[0.5, 0.2, 0.0]]) + u(-0.5, 0.5, 1, 3)})


def mixed(name, **rows):
    """V0 of the world with rows of V1: mixed("field", B=slice(5, 11)) has boxes 5..10 from V1; B=True all of them."""
    v0, v1 = values(name, 0), values(name, 1)
    out = {k: np.array(a) for k, a in v0.items()}
    for k, sl in rows.items():
        sl = slice(None) if sl is True else sl
        out[k][sl] = v1[k][sl]
    return out


def build(name, v):
    """The world from its values: the same call sequence for every value, so the ids agree."""
    art.reset_scene_rng()
    m = v["M"]
    mats = [art.lambertian((0.65, 0.05, 0.05)), art.lambertian((0.73, 0.73, 0.73)), art.lambertian((0.12, 0.45, 0.15)),
            art.metal(v3(m[METAL_ID, :3]), float(m[METAL_ID, 3])), art.dielectric(float(m[GLASS_ID, 4]))]
    light = art.diffuse_light(art.solid_color(7.0, 7.0, 7.0))
    assert [x.id for x in mats + [light]] == list(range(6))
    rect = lambda k, mat: RECT_CLASS[int(v["AX"][k])](*v["R"][k], mat)  # noqa: E731
    box = lambda k, mat: art.box(v3(v["B"][k, :3]), v3(v["B"][k, 3:]), mat)  # noqa: E731
    w = art.hittable_list()
    if name == "room":
        for k, mat in enumerate((mats[2], mats[0], light, mats[1], mats[1], mats[1])):
            w.add(rect(k, mat))
        for k in range(2):
            w.add(art.translate(art.rotate_y(box(k, mats[1 + 2 * k]), float(v["ANG"][k])), v3(v["OFF"][k])))
        w.add(art.constant_medium(art.translate(art.rotate_y(box(2, mats[1]), float(v["ANG"][2])), v3(v["OFF"][2])), float(v["DENS"][0]), (0.9, 0.9, 0.9)))
        w.add(art.constant_medium(art.sphere((3.0, 7.5, 3.0), 1.2, mats[1]), float(v["DENS"][1]), (0.2, 0.4, 0.9)))
    elif name == "field":
        objs = []
        for k in range(16):  # interleaved in the list too; the SAH builder sorts by position anyway
            objs.append(box(k, mats[k % 5]))
            if k % 2 == 0:
                objs.append(art.sphere(v3(v["S"][k // 2, :3]), float(v["S"][k // 2, 3]), mats[(k // 2) % 5]))
            elif k // 2 + 1 < 8:
                objs.append(rect(k // 2 + 1, mats[(k // 2) % 4]))
        objs.append(rect(0, mats[1]))
        w.add(art.bvh_node(objs))
        w.add(rect(8, light))
    else:
        w.add(rect(0, mats[1]))
        w.add(art.translate(box(0, mats[3]), v3(v["OFF"][0])))
    return art.hittable_list(native=art.compile_world(w, 0))


def rect_order(name):
    """scene_rects' row k is values' row rect_order(name)[k] (the compiled order is the world list walked in order)."""
    return np.array([1, 2, 3, 4, 5, 6, 7, 0, 8]) if name == "field" else np.arange(len(values(name, 0)["R"]))


def rect_rows(name, v):
    return np.ascontiguousarray(v["R"][rect_order(name)])


def frame_camera(name):
    at = {"room": ((5.0, 5.0, -13.0), (5.0, 5.0, 0.0)), "field": ((3.0, 7.0, 11.0), (0.0, 0.7, 0.0)), "loose": ((2.0, 4.0, 8.0), (0.0, 0.7, 0.0))}[name]
    return art.camera(at[0], at[1], (0, 1, 0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)


def query_rays(name):
    """256 rays from inside the scene's extent in seeded random directions."""
    lo, hi = {"room": ((1.0, 1.0, -3.0), (9.0, 9.0, 9.0)), "field": ((-5.0, 0.2, -5.0), (5.0, 4.0, 5.0)), "loose": ((-4.0, 0.3, -4.0), (4.0, 4.0, 4.0))}[name]
    rng = np.random.default_rng(11)
    rays = np.zeros((NRAYS, 7))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = rng.uniform(lo, hi, (NRAYS, 3)), rng.normal(size=(NRAYS, 3)), rng.uniform(0, 1, NRAYS)
    return rays


def no_two_planes_of_one_bvh_share_a_coordinate(name, v):
    """The condition on the inputs: per BVH and axis, every rect plane (its k on its normal axis) and every box face is
    at a coordinate of its own."""
    in_bvh = {"room": (range(6), ()), "field": (range(9), range(16)), "loose": ((), ())}[name]  # (world merging puts field's light into the BVH)
    planes = [[], [], []]
    for k in in_bvh[0]:
        planes[{0: 2, 1: 1, 2: 0}[int(v["AX"][k])]].append(v["R"][k, 4])
    for k in in_bvh[1]:
        for a in range(3):
            planes[a] += [v["B"][k, a], v["B"][k, 3 + a]]
    for a in range(3):
        assert len(set(planes[a])) == len(planes[a]), (name, a)


@functools.lru_cache(maxsize=None)
def fresh(name, key="V1"):
    """A world compiled fresh with its frame and what its getters give, computed once and read by every test that compares
    with it.  key "V1": every rect, box and object value from V1; others: see KEYS."""
    v = mixed(name, **KEYS[key])
    no_two_planes_of_one_bvh_share_a_coordinate(name, v)
    b = build(name, v)
    return b, render(b, frame_camera(name), SKY, SIZE), getters(b), v


KEYS = {"V0": {}, "V1": dict(R=True, B=True, ANG=True, OFF=True, DENS=True), "part": dict(B=slice(5, 11), R=slice(2, 5)),
        "objects part": dict(ANG=slice(1, 2), OFF=slice(1, 2)), "mixed kinds": dict(S=True, B=True, M=True)}


def getters(world):
    return art.scene_rects(world), art.scene_boxes(world), art.scene_objects(world), art.scene_spheres(world), art.scene_materials(world)


def same_getters(a, b):
    for (ga, gb) in zip(a[:3] + a[4:], b[:3] + b[4:]):
        assert (bits(ga[0]) == bits(gb[0])).all() and (ga[1] == gb[1]).all()
    assert (bits(a[3]) == bits(b[3])).all()


def start(name):
    """The V0 world, its frame and the condition on its values."""
    v0 = mixed(name)
    no_two_planes_of_one_bvh_share_a_coordinate(name, v0)
    a = build(name, v0)
    return a, render(a, frame_camera(name), SKY, SIZE), v0


def equals_fresh(a, name, key, before):
    b, frame_b, get_b, vb = fresh(name, key)
    ra = render(a, frame_camera(name), SKY, SIZE)
    assert same_render(ra, frame_b), (int((ra[0] != frame_b[0]).sum()), ra[2]["segments"], frame_b[2]["segments"])
    assert not same_render(ra, before) and ra[0].max() > 0 and kernel_of(ra[2]) == kernel_of(before[2])
    hits = same_queries(a, b, query_rays(name))
    assert np.isfinite(hits[:, 0]).sum() > NRAYS // 8 and np.isinf(hits[:, 0]).any()  # the rays cover scene and sky
    same_getters(getters(a), get_b)
    return ra


# ------------------------------------------------------------------------------------------------ 5. equality with a fresh compile
ORDERS = [(n, o) for n in ("room", "field", "loose") for o in (("rects", "boxes", "objects"), ("objects", "boxes", "rects"))]


@pytest.mark.parametrize("name,order", ORDERS, ids=[f"{n}-{'-'.join(k[0] for k in o)}" for n, o in ORDERS])
def test_every_rect_box_and_object_updated_equals_the_fresh_compile(gpu, name, order):
    a, before, v0 = start(name)
    b, _, get_b, v1 = fresh(name)
    (r0, rd0), (b0, bd0), (p0, pd0) = getters(a)[:3]
    assert (bits(r0) == bits(rect_rows(name, v0))).all() and (rd0[:, 0] == v0["AX"][rect_order(name)]).all() and (bits(b0) == bits(v0["B"])).all()
    p1, pd1 = get_b[2]  # the objects' V1: the fresh V1 compile's own
    assert (pd1 == pd0).all() and (name == "field" or (bits(p1) != bits(p0)).any())
    nodes0, refs0 = art.scene_bvh(a)
    assert (len(nodes0) == 0 and len(refs0) == 0) == (name == "loose")  # `loose` has no BVH and no slots
    steps = {"rects": lambda: art.update_rects(a, rect_rows(name, v1)), "boxes": lambda: art.update_boxes(a, v1["B"]), "objects": lambda: art.update_objects(a, p1)}
    for kind in order:
        assert steps[kind]() is None
    equals_fresh(a, name, "V1", before)
    (r, _), (bx, _), (p, pd) = getters(a)[:3]
    assert (bits(r) == bits(rect_rows(name, v1))).all() and (bits(bx) == bits(v1["B"])).all()
    # what update_objects wrote is what the helpers make of V1
    for k in np.flatnonzero(pd[:, 0] == ROTATE_Y):
        chain = int((pd[:k, 0] == ROTATE_Y).sum())
        assert (bits(p[k, :2]) == bits(np.array(art.rotation(v1["ANG"][chain])))).all() and (p[k, 2:] == 0).all()
    for chain, k in enumerate(np.flatnonzero(pd[:, 0] == TRANSLATE)):
        assert (bits(p[k, :3]) == bits(v1["OFF"][chain])).all()
    for chain, k in enumerate(np.flatnonzero(pd[:, 0] == MEDIUM)):
        assert p[k, 0] == art.medium_density(v1["DENS"][chain])
    nodes, refs = art.scene_bvh(a)
    assert (nodes["child"] == nodes0["child"]).all() and (nodes["pad"] == nodes0["pad"]).all() and (refs == refs0).all()


def test_a_prim_and_a_bvh_object_take_nothing_and_a_kind_only_its_fields(gpu):
    a, before, v0 = start("room")
    p0, pd = art.scene_objects(a)
    junk = np.arange(100.0, 100.0 + p0.size).reshape(p0.shape)
    art.update_objects(a, junk)
    p, _ = art.scene_objects(a)
    want = np.array(p0)
    for k, kind in enumerate(pd[:, 0]):
        n = {PRIM: 0, BVH: 0, TRANSLATE: 3, ROTATE_Y: 2, MEDIUM: 1}[int(kind)]
        want[k, :n] = junk[k, :n]
    assert (bits(p) == bits(want)).all() and {PRIM, BVH, TRANSLATE, ROTATE_Y, MEDIUM} == set(pd[:, 0].tolist())
    art.update_objects(a, p0)  # and back: get -> update changes nothing
    assert same_render(render(a, frame_camera("room"), SKY, SIZE), before)


# ------------------------------------------------------------------------------------------------ 6. the tree
def the_boxes_are_the_specified_ones(nodes, refs, spheres, rects, axes, boxes):
    """A leaf's box is refit.h's conservative box of the union of its primitives' f64 boxes (a rect: its extent and
    k -/+ 0.0001 on its normal axis, refit.h rect_box; a box: mn / mx; a sphere: c -/+ r), an inner child's the union of that
    node's live boxes, an empty child's the empty box.  Returns the number of leaves that mix kinds."""
    planes = lambda n, c: (np.array([nodes["lox"][n, c], nodes["loy"][n, c], nodes["loz"][n, c]]),  # noqa: E731
                           np.array([nodes["hix"][n, c], nodes["hiy"][n, c], nodes["hiz"][n, c]]))
    rl, rh = np.zeros((len(rects), 3)), np.zeros((len(rects), 3))
    for k, (r, ax) in enumerate(zip(rects, axes)):
        ka, ia, ib = {0: (2, 0, 1), 1: (1, 0, 2), 2: (0, 1, 2)}[int(ax)]
        rl[k, ia], rh[k, ia], rl[k, ib], rh[k, ib], rl[k, ka], rh[k, ka] = r[0], r[1], r[2], r[3], r[4] - 0.0001, r[4] + 0.0001
    prim_lo = {0: spheres[:, :3] - spheres[:, 3:4], 2: rl, 3: boxes[:, :3]}  # by reference type
    prim_hi = {0: spheres[:, :3] + spheres[:, 3:4], 2: rh, 3: boxes[:, 3:]}
    leaves = inner = mixes = 0
    for n in range(len(nodes)):
        for c in range(4):
            code = int(nodes["child"][n, c])
            lo, hi = planes(n, c)
            if code == -1:
                assert (lo == np.finfo(F32).max).all() and (hi == -np.finfo(F32).max).all()
            elif code < 0:
                first, count = ~code & 0xFFFFFF, (~code >> 24) & 0x7F
                r = refs[first:first + count]
                ty, idx = (r >> 30).tolist(), (r & (2 ** 30 - 1)).tolist()
                wl, wh = conservative_box_np(np.min([prim_lo[t][i] for t, i in zip(ty, idx)], 0), np.max([prim_hi[t][i] for t, i in zip(ty, idx)], 0))
                assert (lo.view(np.int32) == wl.view(np.int32)).all() and (hi.view(np.int32) == wh.view(np.int32)).all(), (n, c)
                leaves += 1
                mixes += len(set(ty)) > 1
            else:
                assert code > n
                live = nodes["child"][code] != -1
                wl = np.array([nodes[f][code][live].min() for f in ("lox", "loy", "loz")])
                wh = np.array([nodes[f][code][live].max() for f in ("hix", "hiy", "hiz")])
                assert (lo == wl).all() and (hi == wh).all(), (n, c)
                inner += 1
    assert leaves >= 8 and inner == len(nodes) - 1  # every node but the root is some node's child
    return mixes


def test_the_refitted_boxes_of_field_are_the_specified_ones(gpu):
    a, before, v0 = start("field")
    v1 = fresh("field")[3]
    nodes0, refs0 = art.scene_bvh(a)
    ax = v0["AX"][rect_order("field")]
    art.update_rects(a, rect_rows("field", v1))
    art.update_boxes(a, v1["B"])
    nodes, refs = art.scene_bvh(a)
    assert len(nodes) == len(nodes0) and (nodes["child"] == nodes0["child"]).all() and (nodes["pad"] == nodes0["pad"]).all() and (refs == refs0).all()
    assert set((refs >> 30).tolist()) == {0, 2, 3}
    changed = sum(int((nodes[f] != nodes0[f]).sum()) for f in ("lox", "hix", "loy", "hiy", "loz", "hiz"))
    assert changed > len(nodes)  # the updates did move the boxes
    assert the_boxes_are_the_specified_ones(nodes, refs, v0["S"], rect_rows("field", v1), ax, v1["B"]) >= 1  # at least one leaf mixes kinds


# ------------------------------------------------------------------------------------------------ 7. a sub-range
def test_a_sub_range_leaves_every_other_record_alone_and_equals_its_fresh_compile(gpu):
    a, before, v0 = start("field")
    v1 = fresh("field")[3]
    r0, b0 = rect_rows("field", v0), v0["B"]
    # values rows 2..4 of R are scene_rects rows 1..3
    assert art.update_rects(a, rect_rows("field", v1)[1:4], first=1) is None and art.update_boxes(a, v1["B"][5:11], first=5) is None
    (r, _), (bx, _) = getters(a)[:2]
    keep_r, keep_b = np.r_[0, 4:9], np.r_[0:5, 11:16]
    assert (bits(r[keep_r]) == bits(r0[keep_r])).all() and (bits(bx[keep_b]) == bits(b0[keep_b])).all()
    assert (bits(r[1:4]) == bits(rect_rows("field", v1)[1:4])).all() and (bits(bx[5:11]) == bits(v1["B"][5:11])).all()
    equals_fresh(a, "field", "part", before)


def test_a_sub_range_of_objects(gpu):
    a, before, v0 = start("room")
    get_b = fresh("room", "objects part")[2]
    p0, pd = art.scene_objects(a)
    p1 = get_b[2][0]
    moved = np.flatnonzero((bits(p1) != bits(p0)).any(1))
    assert moved.tolist() == [5, 6] and pd[5:7, 0].tolist() == [ROTATE_Y, TRANSLATE]  # the second box's chain
    art.update_objects(a, p1[5:7], first=5)
    equals_fresh(a, "room", "objects part", before)


# ------------------------------------------------------------------------------------------------ 8. mixed kinds
@pytest.mark.parametrize("order", [("spheres", "boxes", "materials"), ("materials", "boxes", "spheres")], ids=["s-b-m", "m-b-s"])
def test_spheres_boxes_and_materials_on_one_scene_share_the_refit_state(gpu, order):
    a, before, v0 = start("field")
    v = fresh("field", "mixed kinds")[3]
    steps = {"spheres": lambda: art.update_spheres(a, v["S"]), "boxes": lambda: art.update_boxes(a, v["B"]), "materials": lambda: art.update_materials(a, v["M"])}
    for kind in order:
        steps[kind]()
    equals_fresh(a, "field", "mixed kinds", before)
    nodes, refs = art.scene_bvh(a)
    the_boxes_are_the_specified_ones(nodes, refs, v["S"], rect_rows("field", v), v["AX"][rect_order("field")], v["B"])


# ------------------------------------------------------------------------------------------------ 9. other entry points
def updated_room():
    a, before, v0 = start("room")
    b, frame_b, get_b, v1 = fresh("room")
    art.update_objects(a, get_b[2][0])
    art.update_rects(a, rect_rows("room", v1))
    art.update_boxes(a, v1["B"])
    return a, before, frame_b


def test_radiance_rays_and_render_views_see_the_update(gpu):
    a, before, frame_b = updated_room()
    cam, (w, h, spp) = frame_camera("room"), SIZE
    rays, rng = art.camera_rays(cam, w, h, spp, seed=SEED)
    L = art.radiance_rays(a, rays, rng=rng, spp=1, background=SKY).reshape(-1, spp, 3)
    composed = np.zeros_like(L[:, 0])
    for s in range(spp):
        composed = composed + L[:, s]
    assert (bits(composed) == bits(frame_b[1].reshape(-1, 3))).all() and composed.max() > 0
    frames, sums = art.render_views(a, [cam], w, h, spp, seed=SEED, background=SKY, accum=True)
    assert (frames[0] == frame_b[0]).all() and (bits(sums[0]) == bits(frame_b[1])).all()
    assert not (frames[0] == before[0]).all()


# ------------------------------------------------------------------------------------------------ 10. device tensors
def test_device_tensors_on_a_stream_followed_by_a_render_on_it(gpu):
    import torch
    a, before, v0 = start("room")
    b, frame_b, get_b, v1 = fresh("room")
    cam, (w, h, spp) = frame_camera("room"), SIZE
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        p, r, bx = (torch.from_numpy(np.array(x)).to("cuda") for x in (get_b[2][0], rect_rows("room", v1), v1["B"]))
        assert art.update_objects(a, p) is None and art.update_rects(a, r) is None and art.update_boxes(a, bx) is None  # enqueued on the side stream
        got = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
        sums = torch.zeros((1, h, w, 3), dtype=torch.float64, device="cuda")
        art.render_views(a, [cam], w, h, spp, seed=SEED, background=SKY, out=got, accum=sums)
    side.synchronize()
    assert (got.cpu().numpy()[0] == frame_b[0]).all() and (bits(sums.cpu().numpy()[0]) == bits(frame_b[1])).all()
    same_getters(getters(a), get_b)
    with pytest.raises(ValueError):
        art.update_rects(a, r.to(torch.float32))


def test_timing_returns_positive_milliseconds(gpu):
    import torch
    a, before, v0 = start("room")
    b, frame_b, get_b, v1 = fresh("room")
    times = [art.update_objects(a, torch.from_numpy(np.array(get_b[2][0])).to("cuda"), timing=True), art.update_rects(a, rect_rows("room", v1), timing=True),
             art.update_boxes(a, torch.from_numpy(np.array(v1["B"])).to("cuda"), timing=True)]
    assert all(np.isfinite(t) and 0 < t < 1000 for t in times), times
    assert art.update_boxes(a, np.zeros((0, 6)), timing=True) == 0.0
    assert same_render(render(a, frame_camera("room"), SKY, SIZE), frame_b)


# ------------------------------------------------------------------------------------------------ 11. save and load
def test_an_updated_room_saves_and_loads_as_the_updated_one(gpu, tmp_path):
    from another_raytracer_amd._lib import lib
    a, before, frame_b = updated_room()
    assert lib.rt_scene_dump(a._native, None, 0) == 0  # its graph no longer describes it
    path = tmp_path / "room.art"
    art.save_scene(a, path)
    loaded = art.scene_manager(ASSETS).load(path)
    got = render(loaded.objects, frame_camera("room"), SKY, SIZE)
    assert same_render(got, frame_b) and kernel_of(got[2]) == kernel_of(before[2])
    same_getters(getters(loaded.objects), fresh("room")[2])
