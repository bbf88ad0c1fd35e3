"""Recipe scenes: small caller-built worlds, one per persistent k_paths_g<F, TF, LM> kernel (csrc/kernels.hip
launch_paths_g), for the oracle parity gate of tests/test_gpu_recipe_parity.py.  A plain module: no fixtures, no tests.

A recipe is a *family* -- the smallest world that selects one (F, TF) feature / texture set, built through
another_raytracer_amd.scene after art.reset_scene_rng() from a seeded numpy generator -- in one of three sizes that
select the LDS mode (launch_paths_g_ft):

  LM 1  the family as it is: stacks, world list, object records, BVH nodes, primitive references (and the 112-B leaf
        triangles of a kernel with triangles) fit kPathsGLdsCap = 160 KiB;
  LM 2  `loose` small spheres added at world level with compile.world_merge = 0: each costs sizeof(ObjRec) +
        sizeof(PrimRec80) = 128 B plus its 4-B world slot of the LDS head (paths_g_world_bytes), so the head grows until
        the BVH no longer fits beside it while at least kLdsPartialMinNodes = 64 nodes (8 KiB) still do.  The
        triangle-free families' 150 spheres are a tree of 76 nodes, which fits wherever 64 do, so their LM 2 rows also
        hold 6000 spheres (3020 nodes, 378 KiB; still below the 8192 references of 16-bit codes).  The families with
        pair-aligned leaves (F_LEAF2: more than 8191 primitive references) are LM 2 as they are (112 B of LDS per
        reference would be 900 KiB), and have no LM 1 kernel;
  LM 0  more loose spheres: the head leaves no room for 64 nodes.

The loose counts were chosen from those byte counts and a family's measured window (the head also holds the traversal
stacks, 2 or 4 B x stack rows x 768 lanes, which the ABI does not report); rt_stats names the kernel that ran and the
GPU test requires it to be the row's, so a count that drifts out of its window fails there, not silently.

Exact-t ties: the device's tree gives the reference's closest hit only up to exact-t ties (device.h, scene.cpp), so the
geometry avoids them: every coordinate is a seeded random double, no box face rests in a rect's plane (the boxes float
above the floor by a non-dyadic 0.0371), no primitive is listed twice.  The ground's two triangles share an edge and one
material.  They are tilted: the first version laid them flat at y = 0, and every ground pixel differed from the oracle
(more segments on the GPU) -- not a tie but its cousin: the reference's aabb::hit rejects a box of zero thickness, so its
tree hides an axis-aligned triangle in any node that holds it alone, while the product hoists large primitives out of the
tree and pads its boxes.  Settled by changing the recipe.

Kinds: every primitive carries the primitive and material kinds it stands for; build(keep=kind) gives the same world
with only that kind's primitives (the same seeded coordinates), so "t of the full world == t of the kind's world" says
which rays hit the kind first -- the bookkeeping of the non-triviality checks (tests/test_oracle_dump_scenes.py)."""
import os
from collections import namedtuple

import numpy as np

import another_raytracer_amd as art
from tests.oracle_lib import caller_scene_dump, oracle_register_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKY = (0.7, 0.8, 1.0)
DIM = (0.05, 0.06, 0.08)
View = namedtuple("View", "lookfrom lookat vfov aperture background")
VIEW = View((0.37, 3.1, 8.3), (0.1, 0.9, 0.0), 42.0, 0.0, SKY)
ROOM = View((0.37, 2.7, 8.9), (0.1, 2.1, 0.0), 44.0, 0.0, DIM)
FRAME = (32, 18, 4)  # width, height, samples per pixel of the parity frames and the non-triviality checks


def _v(x):
    return tuple(float(t) for t in x)


_image = None


def earth_image():
    """assets/earthmap.jpg, every 4th texel (256 x 128): the one image the recipes use, registered with the oracle."""
    global _image
    if _image is None:
        full = art.imageio.load_image(os.path.join(ROOT, "assets", "earthmap.jpg"))
        _image = np.ascontiguousarray(full[::4, ::4, :3])
        oracle_register_image(_image)
    return _image


class Builder:
    """Collects a world; keep=None keeps every primitive, keep=kind only the primitives that declare the kind."""

    def __init__(self, seed, keep=None):
        self.rng = np.random.default_rng(seed)
        self.keep = keep
        self.world = art.hittable_list()
        self.kinds = set()

    def prim(self, kinds, make):
        """make() when the primitive is kept, else None.  kinds: its primitive kind and its material kind."""
        self.kinds.update(kinds)
        return make() if self.keep is None or self.keep in kinds else None

    def add(self, obj):
        if obj is not None:
            self.world.add(obj)

    def bvh(self, prims):
        prims = [p for p in prims if p is not None]
        return art.bvh_node(prims, 0.0, 1.0) if prims else None

    # ---- ingredients (coordinates drawn whether or not the primitive is kept: the same geometry under every keep)
    def surface_mats(self, texture=None):
        """lambertian (solid, checker or the given texture), metal, dielectric: (kind, material) choices."""
        r = self.rng
        lam = [art.lambertian(_v(r.uniform(0.2, 0.9, 3))) for _ in range(3)]
        lam.append(art.lambertian(art.checker_texture(_v(r.uniform(0.1, 0.4, 3)), _v(r.uniform(0.6, 0.9, 3)))))
        if texture is not None:
            lam = [art.lambertian(texture)]
        return [("lambertian", m) for m in lam] + [("metal", art.metal(_v(r.uniform(0.5, 1.0, 3)), float(r.uniform(0.0, 0.4)))),
                                                     ("dielectric", art.dielectric(1.5))]

    def ground_triangles(self, mat):
        # tilted: an axis-aligned triangle's box is flat, and aabb.h:16-29 (t_max <= t_min) never passes a flat box, so the
        # reference's tree hides such a triangle wherever a node holds it alone; the product's own tree does not
        a, b, c, d = (-7.13, 0.0, -7.29), (7.31, -0.21, -7.17), (7.19, 0.13, 7.23), (-7.27, -0.17, 7.11)
        return [self.prim(("triangle", "lambertian"), lambda: art.triangle(a, b, c, mat)),
                self.prim(("triangle", "lambertian"), lambda: art.triangle(a, c, d, mat))]

    def triangles(self, n, mats, lo=(-3.0, 0.15, -3.0), hi=(3.0, 2.6, 3.0), size=0.7):
        out = []
        for k in range(n):
            c = self.rng.uniform(lo, hi)
            p = [c + self.rng.uniform(-size, size, 3) for _ in range(3)]
            kind, m = mats[k % len(mats)]
            m = m(p) if callable(m) else m
            out.append(self.prim(("triangle", kind), lambda p=p, m=m: art.triangle(_v(p[0]), _v(p[1]), _v(p[2]), m)))
        return out

    def spheres(self, n, mats, lo=(-3.0, 0.3, -3.0), hi=(3.0, 2.4, 3.0), radius=(0.12, 0.3), moving_every=0):
        out = []
        for k in range(n):
            c, r = self.rng.uniform(lo, hi), float(self.rng.uniform(*radius))
            dy = float(self.rng.uniform(0.1, 0.4))
            kind, m = mats[k % len(mats)]
            if moving_every and k % moving_every == 1:
                out.append(self.prim(("moving_sphere", kind), lambda c=c, r=r, dy=dy, m=m: art.moving_sphere(_v(c), _v(c + (0, dy, 0)), 0.0, 1.0, r, m)))
            else:
                out.append(self.prim(("sphere", kind), lambda c=c, r=r, m=m: art.sphere(_v(c), r, m)))
        return out

    def loose_spheres(self, n):
        """World-level spheres (the LM 2 / LM 0 sizes): small, spread over the floor and the air."""
        mats = self.surface_mats()
        for s in self.spheres(n, mats, lo=(-5.0, 0.12, -5.0), hi=(5.0, 3.2, 4.0), radius=(0.05, 0.11)):
            self.add(s)


# ------------------------------------------------------------------------------------------------ families
def _mesh(b, n, texture=None, bary=False):
    """Triangles only, in one bvh_node: the ground's two and n random ones."""
    if bary:
        img = art.image_texture(earth_image())
        mats = [("lambertian", lambda p: art.lambertian(art.barycentric_image_texture(*[_v(b.rng.uniform(0.0, 1.0, 2)) for _ in range(3)], img)))]
        ground = mats[0][1](None)
    else:
        mats = b.surface_mats(texture)
        ground = art.lambertian(texture if texture is not None else art.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
    b.add(b.bvh(b.ground_triangles(ground) + b.triangles(n, mats)))


def tri_solid(b, n=400):
    _mesh(b, n)


def tri_noise(b, n=400):
    """One noise-textured material on every lambertian triangle; past 2000 triangles on the ground alone (a dump writes
    the perlin tables once per primitive: 9000 noise triangles are 60 MB of text for no other kernel)."""
    if n <= 2000:
        return _mesh(b, n, texture=art.noise_texture(3.0))
    mats = b.surface_mats()
    b.add(b.bvh(b.ground_triangles(art.lambertian(art.noise_texture(3.0))) + b.triangles(n, mats)))


def tri_bary(b, n=400):
    _mesh(b, n, bary=True)


def tri_sphere_noise(b, n=400):
    """Triangles and spheres (some moving) in one bvh_node, one noise-textured ground."""
    noise = art.noise_texture(2.0)
    mats = b.surface_mats()
    b.add(b.bvh(b.ground_triangles(art.lambertian(noise)) + b.triangles(n, mats) + b.spheres(90, mats, moving_every=5)))


def rigid_mesh(b, n=300):
    """translate(rotate_y(bvh_node(triangles))), a floating box, a rect light, an image-textured sphere, a ground rect."""
    mats = b.surface_mats()
    mesh = b.bvh(b.triangles(n, mats, lo=(-2.0, 0.2, -2.0), hi=(2.0, 2.4, 2.0)))
    if mesh is not None:
        b.add(art.translate(art.rotate_y(mesh, 23.0), (0.43, 0.0371, -0.29)))
    ground = art.lambertian(art.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
    b.add(b.prim(("rect", "lambertian"), lambda: art.xz_rect(-7.3, 7.1, -7.2, 7.4, 0.0, ground)))
    white = art.lambertian((0.73, 0.73, 0.73))
    b.add(b.prim(("box", "lambertian"), lambda: art.translate(art.rotate_y(art.box((0.0, 0.0, 0.0), (1.3, 1.9, 1.1), white), -17.0), (-3.4, 0.0371, 0.7))))
    b.add(b.prim(("rect", "diffuse_light"), lambda: art.xy_rect(-1.7, 1.9, 2.9, 4.1, -4.3, art.diffuse_light((6.0, 6.0, 6.0)))))
    earth = art.lambertian(art.image_texture(earth_image()))
    b.add(b.prim(("sphere", "lambertian"), lambda: art.sphere((3.1, 1.07, 0.9), 1.03, earth)))


def _small(n):
    """Thousands of spheres are small ones, so that the walls behind them stay in sight."""
    return {"radius": (0.02, 0.05)} if n > 1000 else {}


def _room(b, wall):
    """Five walls and a light (rects), for a camera at +z looking in."""
    red, green, white = art.lambertian((0.65, 0.05, 0.05)), art.lambertian((0.12, 0.45, 0.15)), art.lambertian((0.73, 0.73, 0.73))
    lam = ("rect", "lambertian")
    b.add(b.prim(lam, lambda: art.yz_rect(-0.11, 5.53, -5.17, 9.3, -4.13, green)))
    b.add(b.prim(lam, lambda: art.yz_rect(-0.13, 5.57, -5.19, 9.3, 4.21, red)))
    b.add(b.prim(lam, lambda: art.xz_rect(-4.3, 4.4, -5.3, 9.3, 0.0, white)))
    b.add(b.prim(lam, lambda: art.xz_rect(-4.3, 4.4, -5.3, 9.3, 5.41, white)))
    b.add(b.prim(lam, lambda: art.xy_rect(-4.3, 4.4, -0.2, 5.6, -5.07, wall)))
    b.add(b.prim(("rect", "diffuse_light"), lambda: art.xz_rect(-1.9, 2.1, -2.3, 1.7, 5.37, art.diffuse_light((9.0, 9.0, 9.0)))))


def rect_room(b, n=150, noise=False):
    """Rects, a bvh_node of spheres (some moving), a glass sphere, a sphere-bounded medium (its boundary is no surface
    of the world, so the fog itself is what a camera ray meets first); solid and checker textures (or a noise wall)."""
    wall = art.lambertian(art.noise_texture(1.5) if noise else art.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
    _room(b, wall)
    b.add(b.bvh(b.spheres(n, b.surface_mats(), lo=(-3.5, 0.35, -4.0), hi=(3.5, 4.6, 3.0), moving_every=7, **_small(n))))
    glass = art.dielectric(1.5)
    b.add(b.prim(("sphere", "dielectric"), lambda: art.sphere((-1.9, 0.93, 3.6), 0.9, glass)))
    b.add(b.prim(("constant_medium", "isotropic"), lambda: art.constant_medium(art.sphere((1.3, 1.23, 4.1), 1.17, glass), 1.1, (0.2, 0.4, 0.9))))


def rect_room_noise(b, n=150):
    rect_room(b, n, noise=True)


def smoke(b, n=150, noise=False):
    """The room with constant_medium over rotated boxes (a non-sphere boundary: F_MEDIA_G) and a bvh_node of spheres."""
    wall = art.lambertian(art.noise_texture(1.5) if noise else art.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
    _room(b, wall)
    white = art.lambertian((0.73, 0.73, 0.73))
    for p1, ang, off, dens, col in (((1.7, 3.3, 1.6), 15.0, (0.6, 0.0371, 1.2), 0.9, (0.0, 0.0, 0.0)),
                                    ((1.6, 1.7, 1.7), -18.0, (-2.9, 0.0371, 2.9), 1.3, (1.0, 1.0, 1.0))):
        b.add(b.prim(("constant_medium", "isotropic"), lambda p1=p1, ang=ang, off=off, dens=dens, col=col: art.constant_medium(
            art.translate(art.rotate_y(art.box((0.0, 0.0, 0.0), p1, white), ang), off), dens, col)))
    b.add(b.bvh(b.spheres(n, b.surface_mats(), lo=(-3.5, 0.35, -4.0), hi=(3.5, 4.6, 0.5), **_small(n))))


def smoke_noise(b, n=150):
    smoke(b, n, noise=True)


def boxes(b, n=150):
    """Boxes, transforms and spheres, no triangles, no box-bounded medium: the Next-Week final's feature set."""
    ground = art.lambertian(art.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
    b.add(b.prim(("rect", "lambertian"), lambda: art.xz_rect(-7.3, 7.1, -7.2, 7.4, 0.0, ground)))
    mats = b.surface_mats()
    for k in range(6):
        c = b.rng.uniform((-3.0, 0.0371, -2.5), (2.0, 0.0371, 2.0))
        p1, ang = b.rng.uniform(0.6, 1.5, 3), float(b.rng.uniform(-40.0, 40.0))
        kind, m = mats[k % len(mats)]
        b.add(b.prim(("box", kind), lambda c=c, p1=p1, ang=ang, m=m: art.translate(art.rotate_y(art.box((0.0, 0.0, 0.0), _v(p1), m), ang), _v(c))))
    cloud = b.bvh(b.spheres(n, mats, lo=(-1.5, 0.0, -1.5), hi=(1.5, 2.0, 1.5), radius=(0.08, 0.2) if n <= 1000 else (0.01, 0.03)))
    if cloud is not None:
        b.add(art.translate(art.rotate_y(cloud, 15.0), (0.3, 2.3, -0.4)))


def spheres_many(b, n=1300, noise=False):
    """More spheres (some moving) in one bvh_node than the LDS scene image has slots (1024): k_paths_g, not k_paths."""
    tex = art.noise_texture(2.5) if noise else art.checker_texture((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))
    ground = art.lambertian(tex)
    prims = [b.prim(("sphere", "lambertian"), lambda: art.sphere((0.0, -1000.0, 0.0), 1000.0, ground))]
    b.add(b.bvh(prims + b.spheres(n, b.surface_mats(), lo=(-4.0, 0.1, -4.0), hi=(4.0, 2.8, 3.5), radius=(0.07, 0.16), moving_every=9)))


def spheres_many_noise(b, n=1300):
    spheres_many(b, n, noise=True)


# more than 8192 primitive references: 16-bit leaf codes need pair-aligned leaves (F_LEAF2), or 32-bit codes
LEAF2_TRIANGLES = 9000
# Loose world-level spheres (132 B of LDS head each, module docstring).  Measured on an MI355X over counts 0..1500: the
# 400-triangle and 1300-sphere families run LM 1 up to 300, LM 2 from 500 to 900 (16-bit stacks) or 300 to 700 (32-bit
# stacks: twice the stack bytes), LM 0 from 1000 (800); the families with F_LEAF2 LM 2 up to 800, LM 0 from 900.
LOOSE0 = 1500
MANY_SPHERES = 6000  # spheres in the triangle-free families' bvh_node for LM 2 (below the 8192 references of 16-bit codes)

Recipe = namedtuple("Recipe", "name family size loose view options kernel media")


def _rows():
    C16, L2 = 128, 256
    mesh, mesh_nt, all_nt = 39, 37, 125
    WM0 = {"compile.world_merge": 0}
    rows = []

    def family(name, fn, kernel_ft, view=VIEW, media=False, options=None, size=None, lm1=True, large=(None, 0), wide=LOOSE0):
        """The family's rows: LM 1 as it is, LM 2 (`_large`: (size, loose spheres)), LM 0 (`_wide`: loose spheres)."""
        base = dict(options or {})
        if lm1:
            rows.append(Recipe(name, fn, size, 0, view, base, kernel_ft + (1,), media))
        rows.append(Recipe(name + "_large", fn, large[0] or size, large[1], view, dict(base, **WM0) if large[1] else base, kernel_ft + (2,), media))
        rows.append(Recipe(name + "_wide", fn, size, wide, view, dict(base, **WM0), kernel_ft + (0,), media))

    no16 = {"render.codes16": 0}
    family("tri_solid", tri_solid, (mesh | C16, 3), large=(None, 700))
    family("tri_noise", tri_noise, (mesh | C16, 15), large=(None, 700))
    family("tri_bary", tri_bary, (mesh | C16, 19), large=(None, 700))
    family("tri_solid_c32", tri_solid, (mesh, 3), options=no16, large=(None, 500))
    family("tri_sphere_noise_c32", tri_sphere_noise, (mesh, 15), options=no16, large=(None, 500))
    family("tri_solid_leaf2", tri_solid, (mesh | C16 | L2, 3), size=LEAF2_TRIANGLES, lm1=False)
    family("tri_bary_leaf2", tri_bary, (mesh | C16 | L2, 19), size=LEAF2_TRIANGLES, lm1=False)
    family("tri_noise_leaf2", tri_noise, (mesh | C16 | L2, 15), size=LEAF2_TRIANGLES, lm1=False)
    family("rigid_mesh", rigid_mesh, (127, 15), large=(None, 600))
    # the triangle-free families' 150 spheres are a tree of fewer than 64 nodes, which always fits: their LM 2 rows grow it
    family("rect_room", rect_room, (mesh_nt | C16, 3), view=ROOM, media=True, large=(MANY_SPHERES, 600))
    family("rect_room_noise", rect_room_noise, (mesh_nt | C16, 15), view=ROOM, media=True, large=(MANY_SPHERES, 600))
    family("rect_room_c32", rect_room, (all_nt, 3), view=ROOM, media=True, options=no16, large=(MANY_SPHERES, 500))
    family("smoke_noise", smoke_noise, (all_nt, 15), view=ROOM, media=True, large=(MANY_SPHERES, 500))
    family("boxes", boxes, (189, 15), large=(MANY_SPHERES, 600))
    family("spheres_many", spheres_many, (1 | C16, 3), large=(None, 700))
    family("spheres_many_noise", spheres_many_noise, (1 | C16, 15), large=(None, 700))
    return rows


RECIPES = {r.name: r for r in _rows()}


def build(recipe, keep=None):
    """The recipe's world (an art.hittable_list) and the kinds its primitives declare.  Not compiled: compile it with
    art.compile_world under the recipe's options (compile.world_merge applies at compile time)."""
    art.reset_scene_rng()
    b = Builder(sum(map(ord, recipe.family.__name__)), keep)
    if recipe.size is None:
        recipe.family(b)
    else:
        recipe.family(b, recipe.size)
    if recipe.loose:
        b.loose_spheres(recipe.loose)
    return b.world, b.kinds


def compiled(recipe, set_option, keep=None):
    """(compiled world, oracle dump text, declared kinds) under the recipe's options, set through `set_option` (the
    `options` fixture, or art.set_option).  The render.* options stay set for the renders that follow."""
    for k, v in recipe.options.items():
        set_option(k, v)
    world, kinds = build(recipe, keep)
    native = art.hittable_list(native=art.compile_world(world, 0))
    return native, caller_scene_dump(native, *recipe.view), kinds


def camera(recipe, W, H):
    v = recipe.view
    return art.camera(v.lookfrom, v.lookat, (0, 1, 0), v.vfov, W / H, v.aperture, 10.0, 0.0, 1.0)


def pixel_centre_rays(view, W, H, time=0.5):
    """camera.h:8-47 for aperture 0 in numpy: the ray through the centre of every pixel of a View (anything with
    lookfrom, lookat, vfov), row-major, (W * H, 7)."""
    v = view
    origin, at = np.array(v.lookfrom, np.float64), np.array(v.lookat, np.float64)
    h = np.tan(np.radians(v.vfov) / 2)
    w = (origin - at) / np.linalg.norm(origin - at)
    u = np.cross((0.0, 1.0, 0.0), w)
    u /= np.linalg.norm(u)
    vv = np.cross(w, u)
    hor, ver = 10.0 * (W / H) * 2 * h * u, 10.0 * 2 * h * vv
    llc = origin - hor / 2 - ver / 2 - 10.0 * w
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    s, t = ((i + 0.5) / (W - 1)).ravel(), ((H - 1 - j + 0.5) / (H - 1)).ravel()
    rays = np.empty((W * H, 7))
    rays[:, :3] = origin
    rays[:, 3:6] = llc + s[:, None] * hor + t[:, None] * ver - origin
    rays[:, 6] = time
    return rays


def query_rays(recipe, n=1024, seed=3):
    """Pixel-centre camera rays of the parity frame plus seeded random rays from around the scene towards it."""
    cam = pixel_centre_rays(recipe.view, FRAME[0], FRAME[1])
    rng = np.random.default_rng(seed)
    extra = np.empty((n - len(cam), 7))
    extra[:, :3] = rng.uniform((-6.0, 0.2, -6.0), (6.0, 5.0, 8.0), (len(extra), 3))
    extra[:, 3:6] = rng.uniform((-3.0, 0.1, -3.0), (3.0, 2.5, 3.0), (len(extra), 3)) - extra[:, :3]
    extra[:, 6] = rng.uniform(0.0, 1.0, len(extra))
    return np.concatenate([cam, extra])
