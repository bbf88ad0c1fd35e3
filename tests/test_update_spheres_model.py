"""The host model of rt_scene_update_spheres' refit (tests/native/sphere_refit_check.cpp, refit.h built with g++): 40
spheres, 7 of them moving, get new centres and radii; sphere_box of each updated record, then refit_child over
refit_levels.  The program checks that every refitted box contains the swept extent of its spheres; this file restates
the boxes in numpy from the printed records: a leaf's box is conservative_box of the union of its spheres' swept boxes
(so each box of the one-node tree is numpy's conservative box of the union), an inner child's the min / max of its node's
boxes, and the root's extent covers every sphere."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def conservative_box_np(mn, mx):
    """refit.h conservative_box in numpy float32 arithmetic."""
    l, h = mn.astype(F32), mx.astype(F32)
    l = np.where(l.astype(np.float64) > mn, np.nextafter(l, F32(-np.inf)), l)
    h = np.where(h.astype(np.float64) < mx, np.nextafter(h, F32(np.inf)), h)
    pad = F32(1e-6) * np.maximum(np.maximum(np.abs(l), np.abs(h)), h - l) + F32(1e-30)
    return l - pad, h + pad


def swept_boxes(s):
    """refit.h sphere_box per record row (cx cy cz r dx dy dz t0 dt flags): the boxes at t = 0 and t = 1 of a moving one."""
    c, r, d, t0, dt, moving = s[:, 0:3], s[:, 3:4], s[:, 4:7], s[:, 7:8], s[:, 8:9], s[:, 9:10] != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        f0, f1 = (0.0 - t0) / dt, (1.0 - t0) / dt
        c0, c1 = c + f0 * d, c + f1 * d
    lo = np.where(moving, np.minimum(c0 - r, c1 - r), c - r)
    hi = np.where(moving, np.maximum(c0 + r, c1 + r), c + r)
    return lo, hi


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("sphere_refit") / "sphere_refit_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "another_raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "sphere_refit_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines()
    assert out.returncode == 0 and lines[0] == "ok", out.stdout
    sph = np.array([[float.fromhex(x) for x in ln.split()[2:11]] + [float(ln.split()[11])] for ln in lines if ln.startswith("S ")])
    trees = {}
    for tag in ("T1", "T2"):
        rows = [ln.split()[1:] for ln in lines if ln.startswith(tag + " ")]
        trees[tag] = {(int(r[0]), int(r[1])): (int(r[2]), np.array([float.fromhex(x) for x in r[3:6]], F32), np.array([float.fromhex(x) for x in r[6:9]], F32))
                      for r in rows}
    assert sph.shape == (40, 10) and int(sph[:, 9].sum()) == 7 and len(trees["T1"]) == 16 and len(trees["T2"]) == 4
    return sph, trees


def same(a, b):
    return (np.asarray(a, F32).view(np.int32) == np.asarray(b, F32).view(np.int32)).all()


def test_every_leaf_box_is_the_conservative_box_of_its_spheres_swept_union(model):
    sph, trees = model
    lo, hi = swept_boxes(sph)
    leaves = 0
    for tree in trees.values():
        for (n, c), (code, blo, bhi) in tree.items():
            if code >= 0 or code == -1:
                continue
            first, count = ~code & 0xFFFFFF, (~code >> 24) & 0x7F
            wl, wh = conservative_box_np(lo[first:first + count].min(0), hi[first:first + count].max(0))
            assert same(blo, wl) and same(bhi, wh), (n, c)
            assert (blo < lo[first:first + count]).all() and (bhi > hi[first:first + count]).all()
            leaves += 1
    assert leaves == 14


def test_inner_boxes_are_the_min_and_max_of_their_nodes_and_the_root_covers_everything(model):
    sph, trees = model
    t1 = trees["T1"]
    lo, hi = swept_boxes(sph)
    for c in range(3):
        code, blo, bhi = t1[(0, c)]
        assert code == c + 1
        live = [t1[(code, k)] for k in range(4) if t1[(code, k)][0] != -1]
        assert len(live) == (4 if c < 2 else 2)
        assert same(blo, np.min([b[1] for b in live], 0)) and same(bhi, np.max([b[2] for b in live], 0))
    fmax = np.finfo(F32).max
    for key in ((0, 3), (3, 2), (3, 3)):  # empty slots keep the builder's empty box
        assert t1[key][0] == -1 and (t1[key][1] == fmax).all() and (t1[key][2] == -fmax).all()
    # the root of either tree: min / max over its live boxes covers the union of every sphere's swept box, and is no
    # looser than the union's own conservative box padded once more (each level pads at most once: leaves only)
    for tag, tree in trees.items():
        live = [tree[(0, k)] for k in range(4) if tree[(0, k)][0] != -1]
        rlo, rhi = np.min([b[1] for b in live], 0), np.max([b[2] for b in live], 0)
        assert (rlo < lo.min(0)).all() and (rhi > hi.max(0)).all(), tag
        wl, wh = conservative_box_np(lo.min(0), hi.max(0))
        assert (rlo >= wl).all() and (rhi <= wh).all(), tag  # a leaf's pad is at most the union's: smaller magnitudes and extents
    # the one-node tree whose four leaves hold everything: the union of numpy's conservative leaf boxes is the root
    t2 = trees["T2"]
    want = [conservative_box_np(lo[10 * c:10 * c + 10].min(0), hi[10 * c:10 * c + 10].max(0)) for c in range(4)]
    assert same(np.min([t2[(0, c)][1] for c in range(4)], 0), np.min([w[0] for w in want], 0))
    assert same(np.max([t2[(0, c)][2] for c in range(4)], 0), np.max([w[1] for w in want], 0))


def test_the_moving_spheres_boxes_cover_both_ends_of_the_shutter(model):
    sph, _ = model
    lo, hi = swept_boxes(sph)
    mov = sph[:, 9] != 0
    assert (sph[mov][:, 4:7] != 0).any(1).all()
    k = 13  # x motion of -0.75 over the unit shutter
    assert lo[k, 0] == sph[k, 0] - 0.75 - sph[k, 3] and hi[k, 0] == sph[k, 0] + sph[k, 3]
    k = 25  # shutter [0.25, 0.75]: the centre at t = 0 is c - 0.5 d, at t = 1 c + 1.5 d
    assert lo[k, 2] == sph[k, 2] - 0.5 * 0.3 - sph[k, 3] and hi[k, 2] == sph[k, 2] + 1.5 * 0.3 + sph[k, 3]
