"""another_raytracer_amd — MI355X-native drop-in for the ray_color / BVH / scatter hot path of
blackccpie/another_raytracer.

The Python surface mirrors the reference's own classes so a user of `src/main.cpp` finds the same calls:

    from another_raytracer_amd import scene_manager, scene_alias, camera, engine, engine_mode, imageio
    world = scene_manager().build(scene_alias.random)          # scene_manager.cpp:260-355
    cam = camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    eng = engine(cam, engine_mode.parallel_stripes, width=W, height=H, samples_per_pixel=100)  # engine.h:22
    eng.set_scene(world.objects, world.background)               # engine.h:24-28
    ms = eng.run(image)                                          # engine.h:30-54, image: uint8 (H, W, 3)
    imageio.save_image("output.png", W, H, 3, image)             # imageio.cpp:17-20

Scenes can also be assembled object by object with the reference's constructors (sphere, moving_sphere, triangle,
xy_rect, xz_rect, yz_rect, box, hittable_list, bvh_node, translate, rotate_y, constant_medium; lambertian, metal,
dielectric, diffuse_light; solid_color, checker_texture, noise_texture, image_texture, barycentric_image_texture) and
OBJ/MTL meshes (mesh().parse(path) / .build(), mesh.h) — see scene.py.
Ray queries against a compiled scene -- closest hits with the whole hit_record, or any-hit occlusion with a per-ray
t_max, on numpy arrays or device tensors: query_rays(world.objects, rays, ...); the path-traced radiance along
caller-given rays (other camera models, probes, lightmaps): radiance_rays(world, rays, spp=...), and the renderer's own
camera rays as data: camera_rays(cam, W, H, spp) -- see rays.py.  Many cameras of one scene in one persistent launch, every
frame equal to engine.run's: render_views(world, cams, W, H, spp) -- see views.py.  New vertices for a compiled scene's
triangles with a BVH refit on the device (animated or optimised meshes): update_triangles(world, p); new centres and radii
for its spheres: update_spheres(world, s) -- see deform.py.  New values for its materials and textures (colours, fuzz,
ir, noise scale): update_materials(world, m), update_textures(world, t), and new bytes for its image textures:
update_texels(world, image, texels) -- see appearance.py.  New extents for its rects
and boxes, and new offsets, angles and densities for its translate, rotate_y and constant_medium objects (rigid animation
without a refit): update_rects, update_boxes, update_objects -- see rigid.py.  The exact gradient of radiance_rays'
radiance with respect to the solid texture colours, the metal albedos and the background -- and, with texels=True, every
texel of the scene's image textures: radiance_grad(world, rays, weights), render_grad, and the torch operation
differentiable_radiance -- see grad.py.
All compute runs in libart.so (HIP, gfx950) behind include/art.h.
"""
from ._lib import RTError, get_option, lib, set_option  # noqa: F401  (fails loudly when libart.so is missing)
from .engine import camera, denoise, engine, engine_mode, tracer_constants  # noqa: F401
from .scene import (  # noqa: F401
    barycentric_image_texture, box, bvh_node, checker_texture, constant_medium, dielectric, diffuse_light, hittable_list, image_texture,
    lambertian, mesh, metal, moving_sphere, noise_texture, random_double, rotate_y, scene, scene_alias, scene_manager,
    solid_color, sphere, translate, triangle, xy_rect, xz_rect, yz_rect, reset_scene_rng, save_scene, compile_world,
)
from .rays import HitRecords, camera_rays, query_rays, radiance_rays  # noqa: F401
from .views import render_views  # noqa: F401
from .deform import scene_bvh, scene_lds_image, scene_spheres, scene_triangles, update_spheres, update_triangles  # noqa: F401
from .appearance import (  # noqa: F401
    scene_images, scene_materials, scene_texels, scene_textures, update_materials, update_texels, update_textures,
)
from .rigid import (  # noqa: F401
    OBJ_BVH, OBJ_MEDIUM, OBJ_PRIM, OBJ_ROTATE_Y, OBJ_TRANSLATE, medium_density, rotation, scene_boxes, scene_objects, scene_rects, update_boxes,
    update_objects, update_rects,
)
from .grad import differentiable_radiance, radiance_grad, render_grad  # noqa: F401
from . import imageio  # noqa: F401

__all__ = [
    "RTError", "set_option", "get_option", "camera", "denoise", "engine", "engine_mode", "tracer_constants", "scene", "scene_alias", "scene_manager",
    "query_rays", "radiance_rays", "radiance_grad", "render_grad", "differentiable_radiance", "camera_rays", "render_views", "scene_triangles", "update_triangles", "scene_bvh", "scene_spheres", "update_spheres", "scene_lds_image", "scene_materials", "scene_textures", "update_materials", "update_textures", "scene_images", "scene_texels", "update_texels", "scene_rects", "scene_boxes", "scene_objects", "update_rects", "update_boxes", "update_objects", "rotation", "medium_density",
    "OBJ_PRIM", "OBJ_BVH", "OBJ_TRANSLATE", "OBJ_ROTATE_Y", "OBJ_MEDIUM", "HitRecords", "compile_world", "hittable_list", "bvh_node", "sphere", "moving_sphere", "triangle", "xy_rect", "xz_rect", "yz_rect", "box",
    "translate", "rotate_y", "constant_medium", "lambertian", "metal", "dielectric", "diffuse_light", "solid_color",
    "checker_texture", "noise_texture", "image_texture", "barycentric_image_texture", "mesh", "random_double", "reset_scene_rng", "imageio", "save_scene",
]
