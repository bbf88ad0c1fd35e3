"""Animating a rigid scene (rt_scene_update_rects / _boxes / _objects, include/art.h): new extents for a compiled scene's
rects and boxes, and new parameters for the objects that place them -- where a translate stands, how a rotate_y is turned,
how dense a constant_medium is -- where a new scene would cost a graph, a full SAH build and an upload.  The Cornell box,
the Cornell smoke box, the simple-light scene and the Next-Week final scene are made of these.

    world = art.scene_manager().build("6")               # the Cornell smoke box
    P, desc = art.scene_objects(world)                    # (n, 4) float64: the objects' parameters; desc: kind, a, b, world slot
    turn = np.flatnonzero(desc[:, 0] == art.OBJ_ROTATE_Y)
    P[turn[0], :2] = art.rotation(30.0)                   # sin, cos as a compile of rotate_y(x, 30) makes them
    P[desc[:, 0] == art.OBJ_MEDIUM, 0] = art.medium_density(0.02)
    art.update_objects(world, P)                          # one small launch: no box depends on them
    R, _ = art.scene_rects(world)                         # (n, 5) float64: a0, a1, b0, b1, k
    R[2, :4] = 163, 393, 177, 382                         # a wider ceiling light
    art.update_rects(world, R[2:3], first=2)              # then a refit of every BVH box on the device

Object rows are the compiled object list: the world list walked in order, a wrapper numbered after what it wraps (for
constant_medium(translate(rotate_y(box))): the box, the rotate_y, the translate, the medium), a run of world entries that
compiling merged into one BVH being one object.  A record takes what its kind uses; everything else in a row is ignored
and stays, so get -> update changes nothing.  Every later call gives the bits a scene compiled fresh with the same values
gives (rects and boxes: up to the exact-t ties any two trees can differ in).
"""
import math

import numpy as np

from . import _update

RECT_DOUBLES, BOX_DOUBLES, OBJECT_DOUBLES = 5, 6, 4   # art.h RT_RECT_DOUBLES, RT_BOX_DOUBLES, RT_OBJECT_DOUBLES
OBJ_PRIM, OBJ_BVH, OBJ_TRANSLATE, OBJ_ROTATE_Y, OBJ_MEDIUM = range(5)   # art.h RT_OBJ_*


def scene_rects(world):
    """rt_scene_rects_get: (values, desc) -- values (n, 5) float64: a0, a1, b0, b1, k as the scene holds them now (xy_rect:
    x0, x1, y0, y1, k; xz_rect: x0, x1, z0, z1, k; yz_rect: y0, y1, z0, z1, k); desc (n, 2) int32: axis (0 xy_rect, 1
    xz_rect, 2 yz_rect), material id.  Compiled order: the order the rects are met walking the world list.  Needs no device
    unless the scene has been updated."""
    return _update.get(world, "scene_rects", ((RECT_DOUBLES,), np.float64), ((2,), np.int32))


def scene_boxes(world):
    """rt_scene_boxes_get: (values, desc) -- values (n, 6) float64: min xyz, max xyz; desc (n, 1) int32: material id.
    Compiled order, a box under translate / rotate_y or inside a constant_medium included."""
    return _update.get(world, "scene_boxes", ((BOX_DOUBLES,), np.float64), ((1,), np.int32))


def scene_objects(world):
    """rt_scene_objects_get: (values, desc) -- values (n, 4) float64: an object's parameters p (a translate's offset xyz; a
    rotate_y's sin, cos; a constant_medium's -1 / density; 0 where the kind uses nothing); desc (n, 4) int32: kind (OBJ_PRIM,
    OBJ_BVH, OBJ_TRANSLATE, OBJ_ROTATE_Y, OBJ_MEDIUM), a (a prim's primitive reference type << 30 | index, a BVH's root
    node, a wrapper's child object), b (a medium's phase material id, a BVH's hoisted-leaf code or -1), the object's slot
    in the world list or -1 for one that another object wraps."""
    return _update.get(world, "scene_objects", ((OBJECT_DOUBLES,), np.float64), ((4,), np.int32))


def update_rects(world, v, first=0, stream=None, timing=False):
    """rt_scene_update_rects: v holds rows (a0, a1, b0, b1, k) for rects [first, first + n), shape (n, 5) float64 in
    scene_rects' order; every BVH box is then refitted on the device.  Axis and material stay.

    v, stream and timing are update_spheres': a numpy array copies and blocks (a non-finite value is refused), a contiguous
    float64 torch tensor on the scene's device is read in place on `stream` (default: torch's current stream) and is not
    inspected; timing=True returns the device time in milliseconds."""
    return _update.update(world, v, "v", ((RECT_DOUBLES,),), "shape (n, 5): a0, a1, b0, b1, k per rect", "update_rects", first, stream, timing)


def update_boxes(world, v, first=0, stream=None, timing=False):
    """rt_scene_update_boxes: v holds rows (min xyz, max xyz) for boxes [first, first + n), shape (n, 6) float64 in
    scene_boxes' order; every BVH box is then refitted on the device.  The material stays.  v, stream and timing as
    update_rects."""
    return _update.update(world, v, "v", ((BOX_DOUBLES,),), "shape (n, 6): min xyz, max xyz per box", "update_boxes", first, stream, timing)


def update_objects(world, v, first=0, stream=None, timing=False):
    """rt_scene_update_objects: v holds rows of four parameters for objects [first, first + n), shape (n, 4) float64 in
    scene_objects' order.  A translate takes v[:3] (the offset), a rotate_y v[:2] (sin and cos: rotation(degrees)), a
    constant_medium v[0] (medium_density(d)); a prim and a BVH take nothing.  Nothing is refitted -- a transformed object
    has no box -- so this is one small launch however large the mesh under the transform is.  v, stream and timing as
    update_rects."""
    return _update.update(world, v, "v", ((OBJECT_DOUBLES,),), "shape (n, 4): the object's parameters p", "update_objects", first, stream, timing)


def rotation(degrees):
    """(sin, cos) as compiling rotate_y(x, degrees) makes them, bit for bit: the reference's degrees * pi / 180.0 in that
    order (hittable.cpp:27), then libm's sin and cos."""
    radians = float(degrees) * math.pi / 180.0
    return math.sin(radians), math.cos(radians)


def medium_density(d):
    """A constant_medium's parameter for density d as compiling makes it: -1 / d (constant_medium.h:14)."""
    return -1.0 / float(d)
