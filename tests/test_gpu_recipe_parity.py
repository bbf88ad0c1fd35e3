"""Oracle parity for caller-built scenes on every persistent k_paths_g<F, TF, LM> kernel.

tests/test_gpu_parity.py renders the twelve builtin scenes, which run ten of the library's k_paths_g kernels.  The rest
run only for scenes a caller builds; here each of them (tests/recipes.py: one recipe row per kernel) renders a recipe
scene and must equal, bit for bit (RGB8, f64 radiance sums, segment count), the CPU oracle reading the same scene from
its canonical dump (oracle/restate.cpp, pcg mode) -- and rt_stats must name the row's kernel, so the test sees the
intended kernel run.  The same frame through the per-depth wavefront kernels (the bounce<> instantiations) and, for
media-free recipes, 1024 closest-hit ray queries (the ray kernels chosen by with_ray_features) must equal the oracle too.
"""
import numpy as np
import pytest

import another_raytracer_amd as art
from tests import recipes
from tests.oracle_lib import oracle_render, oracle_render_adaptive, oracle_render_rows, oracle_trace_rays
from tests.update_common import bits

pytestmark = pytest.mark.gpu

ROWS = list(recipes.RECIPES)


def render(world, recipe, W, H, spp, mode=art.engine_mode.single, wavefront=False, max_depth=50, band=None):
    """tests/test_gpu_parity.py gpu_render for a compiled caller-built world under the recipe's view."""
    eng = art.engine(recipes.camera(recipe, W, H), mode, width=W, height=H, samples_per_pixel=spp, precision="f64", seed=0,
                     max_depth=max_depth)
    eng.set_scene(world, recipe.view.background)
    eng.wavefront = wavefront
    band_rows, band_count, band_index = band or (None, 1, 0)
    rows = H if band is None else len(eng.local_rows(band_rows, band_count, band_index))
    img, acc = np.zeros((rows, W, 3), np.uint8), np.zeros((rows, W, 3), np.float64)
    if mode == art.engine_mode.adaptive:
        eng.run(img)
    else:
        eng.run(img, accum=acc, band_rows=band_rows, band_count=band_count, band_index=band_index)
    return {"rgb": img, "acc": acc, "segments": eng.stats["segments"], "stats": eng.stats, "engine": eng}


def kernel(stats):
    return stats["kernel_features"], stats["kernel_textures"], stats["kernel_lds_mode"]


def same(g, o):
    return np.array_equal(g["rgb"], o["rgb"]) and np.array_equal(bits(g["acc"]), bits(o["acc"])) and g["segments"] == o["segments"]


def differing(g, o):
    return f"{int((bits(g['acc']) != bits(o['acc'])).any(-1).sum())} pixels differ, segments {g['segments']} vs {o['segments']}"


@pytest.mark.parametrize("name", ROWS)
def test_recipe_matches_oracle_on_its_kernel(gpu, options, name):
    recipe = recipes.RECIPES[name]
    world, dump, _ = recipes.compiled(recipe, options)
    W, H, spp = recipes.FRAME
    o = oracle_render(dump, W, H, spp, mode="pcg")
    g = render(world, recipe, W, H, spp)
    print(f"{name}: kernel {kernel(g['stats'])} variant {g['stats']['extend_variant']}, {differing(g, o)}")
    assert g["stats"]["extend_variant"] == 4 and kernel(g["stats"]) == recipe.kernel, (kernel(g["stats"]), recipe.kernel)
    assert same(g, o), differing(g, o)
    wf = render(world, recipe, W, H, spp, wavefront=True)  # the per-depth kernels: bounce<> of the scene's features
    assert wf["stats"]["extend_variant"] == 0
    assert same(wf, o), differing(wf, o)
    if not recipe.media:  # closest hits of the ray kernels (a medium's draws belong to rt_trace_rays' contract, not rt_query_rays')
        rays = recipes.query_rays(recipe)
        hits = art.query_rays(world, rays)
        t, nrm = oracle_trace_rays(dump, rays)
        assert np.isfinite(t).mean() > 0.3
        assert np.array_equal(bits(np.asarray(hits.t)), bits(t))
        assert np.array_equal(bits(np.asarray(hits.normal)), bits(nrm))  # a miss: +inf and a zero normal on both sides


TWO = ["rigid_mesh", "rect_room"]


@pytest.mark.parametrize("name", TWO)
@pytest.mark.parametrize("W,H,spp,max_depth", [(13, 70, 2, 50), (32, 18, 4, 1)])
def test_ragged_frame_and_one_bounce(gpu, options, name, W, H, spp, max_depth):
    recipe = recipes.RECIPES[name]
    world, dump, _ = recipes.compiled(recipe, options)
    o = oracle_render(dump, W, H, spp, mode="pcg", max_depth=max_depth)
    for wavefront in (False, True):
        g = render(world, recipe, W, H, spp, wavefront=wavefront, max_depth=max_depth)
        assert wavefront or kernel(g["stats"]) == recipe.kernel
        assert same(g, o), (wavefront, differing(g, o))


@pytest.mark.parametrize("name", TWO)
def test_adaptive_matches_oracle(gpu, options, name):
    recipe = recipes.RECIPES[name]
    world, dump, _ = recipes.compiled(recipe, options)
    W, H, spp = 24, 12, 8
    g = render(world, recipe, W, H, spp, mode=art.engine_mode.adaptive)
    o = oracle_render_adaptive(dump, W, H, spp, mode="pcg")
    assert np.array_equal(g["rgb"], o["rgb"])
    assert g["segments"] == o["segments"]


def test_band_partitioned_large_recipe_matches_oracle_rows(gpu, options):
    recipe = recipes.RECIPES["rigid_mesh_large"]
    world, dump, _ = recipes.compiled(recipe, options)
    W, H, spp = recipes.FRAME
    for band in range(2):
        g = render(world, recipe, W, H, spp, band=(4, 2, band))
        rows = g["engine"].local_rows(4, 2, band)
        assert kernel(g["stats"]) == recipe.kernel
        assert same(g, oracle_render_rows(dump, W, H, spp, rows)), band
