"""What the GPU tests of the scene-update calls (tests/test_gpu_update_*.py) share: the frame and query sizes, bit
comparison, the small worlds' ingredients, rendering a compiled world and comparing two of them.  A plain module: no
fixtures, no tests."""
import os

import numpy as np

import another_raytracer_amd as art

W, H, SPP = 64, 36, 8
NQ = 4096
SKY = (0.6, 0.7, 0.9)
F_LEAF2 = 256
F32 = np.float32
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets")

# csrc/layout.h: the LDS scene image's planes (ART_LDS_NODE_CAP 272, 1024 slots, 512 material entries), tile_lists.h TileReps
NODE_CAP, SLOT_CAP = 272, 1024
OFF_SPH = 10 * NODE_CAP * 16
OFF_MOV = OFF_SPH + 2 * SLOT_CAP * 16
OFF_REF = OFF_MOV + SLOT_CAP * 8
OFF_MATIDX = OFF_REF + SLOT_CAP * 4
OFF_MAT = OFF_MATIDX + SLOT_CAP * 2
OFF_INVR = OFF_MAT + 512 * 32
IMAGE_BYTES = OFF_INVR + SLOT_CAP * 8
REPS_BYTES = 4 + 2 * SLOT_CAP + 12


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def quant(a):
    """Multiples of 2^-20: c + d and (c + d) - c of a moving sphere are then exact, so the fresh compile's center1 - center0
    is the motion the updated scene kept."""
    return np.round(np.asarray(a, np.float64) * 2.0 ** 20) / 2.0 ** 20


def v3(x):
    return tuple(float(t) for t in x)


# ------------------------------------------------------------------------------------------------ ingredients of the worlds
def grid_triangles(n=12):
    """An n x n height field over [-3, 3]^2 with seeded random heights in [0, 1.5]: 2 n^2 triangles (288), no coplanar
    neighbours."""
    rng = np.random.default_rng(7)
    xs = np.linspace(-3.0, 3.0, n + 1)
    y = rng.uniform(0.0, 1.5, (n + 1, n + 1))
    v = lambda i, j: (xs[i], y[i, j], xs[j])  # noqa: E731
    tris = []
    for i in range(n):
        for j in range(n):
            tris.append((v(i, j), v(i + 1, j), v(i, j + 1)))
            tris.append((v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)))
    return np.array(tris, np.float64)


def make_sphere(s, d, mat):
    if d.any():
        return art.moving_sphere(v3(s[:3]), v3(s[:3] + d), 0.0, 1.0, float(s[3]), mat)
    return art.sphere(v3(s[:3]), float(s[3]), mat)


def image_spheres():
    """The `image` worlds' 49 spheres (S0 (49, 4), D (49, 3)): a ground sphere of radius 100 and 48 small ones, 6 of them
    moving along y."""
    rng = np.random.default_rng(21)
    s0, d = np.zeros((49, 4)), np.zeros((49, 3))
    s0[0] = (0.0, -100.0, 0.0, 100.0)
    k = 1
    for i in range(8):
        for j in range(6):
            r = rng.uniform(0.2, 0.3)
            s0[k] = (-3.5 + i + rng.uniform(-0.2, 0.2), r, -2.5 + j + rng.uniform(-0.2, 0.2), r)
            if k % 8 == 3:
                d[k, 1] = 0.25 + 0.125 * (k % 3)  # y motion over the unit shutter: the image's moving spheres
            k += 1
    return quant(s0), d


def frame_camera(name):
    at = {"image": ((0.0, 3.0, 9.0), (0.0, 0.3, 0.0)), "mixed": ((1.0, 7.0, 12.0), (0.0, 1.5, 0.0)),
          "xform_media": ((1.0, 5.0, 13.0), (0.0, 1.0, 0.0)), "side": ((9.0, 4.0, 3.0), (0.0, 1.0, 0.0))}[name]
    return art.camera(at[0], at[1], (0, 1, 0), 40.0, W / H, 0.0, 10.0, 0.0, 1.0)


# ------------------------------------------------------------------------------------------------ frames and queries
def engine_for(world, cam, background=SKY, size=(W, H, SPP), **form):
    eng = art.engine(cam, art.engine_mode.single, width=size[0], height=size[1], samples_per_pixel=size[2], seed=5)
    for k, v in form.items():
        setattr(eng, k, v)
    eng.set_scene(world, background)
    return eng


def render(world, cam, background=SKY, size=(W, H, SPP), **form):
    eng = engine_for(world, cam, background, size, **form)
    img, acc = np.zeros((size[1], size[0], 3), np.uint8), np.zeros((size[1], size[0], 3), np.float64)
    eng.run(img, accum=acc)
    return img, acc, eng.stats


def same_render(a, b):
    return (a[0] == b[0]).all() and (bits(a[1]) == bits(b[1])).all() and a[2]["segments"] == b[2]["segments"]


def kernel_of(stats):
    return stats["kernel_features"], stats["kernel_textures"], stats["kernel_lds_mode"], stats["extend_variant"]


def same_queries(a, b, rays, **kw):
    """Closest hits and occlusion bytes of `rays` agree between the worlds a and b; returns a's hit records."""
    ra, rb = art.query_rays(a, rays, **kw).records, art.query_rays(b, rays, **kw).records
    oa, ob = art.query_rays(a, rays, any_hit=True, **kw), art.query_rays(b, rays, any_hit=True, **kw)
    assert ra.shape == (len(rays), 12)
    assert (bits(ra) == bits(rb)).all(), int((bits(ra) != bits(rb)).any(1).sum())
    assert (oa == ob).all()
    return ra


# ------------------------------------------------------------------------------------------------ the tree
def covered_slots(nodes, n_refs):
    """Which leaf slots some node's leaf holds (scene_bvh's nodes)."""
    seen = np.zeros(n_refs, bool)
    for code in nodes["child"].ravel():
        code = int(code)
        if code < -1:
            first, count = ~code & 0xFFFFFF, (~code >> 24) & 0x7F
            seen[first:first + count] = True
    return seen


def conservative_box_np(mn, mx):
    """refit.h conservative_box in numpy float32 arithmetic."""
    l, h = mn.astype(F32), mx.astype(F32)
    l = np.where(l.astype(np.float64) > mn, np.nextafter(l, F32(-np.inf)), l)
    h = np.where(h.astype(np.float64) < mx, np.nextafter(h, F32(np.inf)), h)
    pad = F32(1e-6) * np.maximum(np.maximum(np.abs(l), np.abs(h)), h - l) + F32(1e-30)
    return l - pad, h + pad
