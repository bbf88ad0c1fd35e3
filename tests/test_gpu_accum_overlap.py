"""A split whole-image k_paths pass (csrc/pass_plan.h split_pass, renderer.hip trace_samples; option
render.accum_overlap): the pass runs as a head and a tail launch and the head's radiance records are summed on a second
stream while the tail traces.

Scene 1 at 72x40 (partial 8x8 tiles in both directions), 24 spp, max_depth 50, with the split forced (option 2): the
RGB8 frame, the f64 sums and the segment count are bit-identical to the unsplit render (option 0) and to the oracle, over
several planned passes, on a band, and on a caller's stream with device buffers.  A progressive render, the adaptive
levels' pixel lists and a k_paths_g scene are never split; auto (option 1) leaves a frame this small at one launch per
pass; RT_PROFILE's marks count and time the k_paths launches alone."""
import functools

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd.distributed import band_rows_of
from tests.oracle_lib import oracle_render

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH = 72, 40, 24, 50


def engine_of(scene, W, H, spp, mode=None, samples_per_pass=0):
    world = art.scene_manager().build(scene)
    c = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    eng = art.engine(c, mode or art.engine_mode.single, width=W, height=H, samples_per_pixel=spp, precision="f64", seed=0,
                     max_depth=DEPTH, samples_per_pass=samples_per_pass)
    eng.set_scene(world.objects, world.background)
    return eng


@functools.lru_cache(maxsize=None)
def render(overlap, scene="1", W=W, H=H, spp=SPP, samples_per_pass=0, bands=None, profile=False, adaptive=False):
    """One host-buffer render under option render.accum_overlap = overlap; bands = (band_rows, band_count, band_index)."""
    eng = engine_of(scene, W, H, spp, art.engine_mode.adaptive if adaptive else None, samples_per_pass)
    kw = dict(band_rows=bands[0], band_count=bands[1], band_index=bands[2]) if bands else {}
    rows = len(band_rows_of(H, *bands)) if bands else H
    img = np.zeros((rows, W, 3), np.uint8)
    acc = None if adaptive else np.zeros((rows, W, 3), np.float64)
    art.set_option("render.accum_overlap", overlap)
    try:
        eng.run(img, accum=acc, profile=profile, **kw)
    finally:
        art.set_option(None, 0)
    return {"rgb": img, "acc": acc, "segments": eng.stats["segments"], "stats": eng.stats}


def same(a, b):
    return a["acc"].tobytes() == b["acc"].tobytes() and np.array_equal(a["rgb"], b["rgb"]) and a["segments"] == b["segments"]


def test_split_equals_unsplit_and_the_oracle(gpu):
    on, off = render(2), render(0)
    assert on["stats"]["extend_variant"] == 3 and off["stats"]["extend_variant"] == 3
    assert off["stats"]["passes"] == 1 and on["stats"]["passes"] == 2  # one planned pass, two launches
    assert on["stats"]["samples_per_pass"] == SPP == off["stats"]["samples_per_pass"]  # the planned k
    assert same(on, off)
    assert same(on, oracle_render("1", W, H, SPP, mode="pcg", max_depth=DEPTH))


def test_three_planned_passes_each_split(gpu):
    many = render(2, samples_per_pass=10)  # 24 samples spread over three passes of 8
    assert many["stats"]["samples_per_pass"] == 8 and many["stats"]["passes"] == 6
    assert same(many, render(0))


def test_band_equals_the_rows_of_the_unbanded_frame(gpu):
    band = render(2, bands=(8, 2, 1))
    rows = band_rows_of(H, 8, 2, 1)
    whole = render(0)
    assert band["stats"]["passes"] == 2
    assert band["acc"].tobytes() == whole["acc"][rows].tobytes() and np.array_equal(band["rgb"], whole["rgb"][rows])
    assert band["segments"] == render(0, bands=(8, 2, 1))["segments"]


def test_callers_stream_and_device_buffers(gpu):
    import torch
    eng = engine_of("1", W, H, SPP)
    side = torch.cuda.Stream()
    art.set_option("render.accum_overlap", 2)
    try:
        with torch.cuda.stream(side):
            img = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            acc = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
            eng.run(img, accum=acc, stream=side.cuda_stream)
        side.synchronize()  # the caller's stream alone: the second stream's work is ordered before its end
    finally:
        art.set_option(None, 0)
    off = render(0)
    assert eng.stats["passes"] == 2 and eng.stats["segments"] == off["segments"]
    assert np.array_equal(img.cpu().numpy(), off["rgb"]) and acc.cpu().numpy().tobytes() == off["acc"].tobytes()


def test_progressive_render_is_not_split(gpu):
    frames = {}
    for overlap in (2, 0):
        eng = engine_of("1", W, H, SPP)
        img, acc, seen = np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.float64), []
        art.set_option("render.accum_overlap", overlap)
        try:
            eng.run_progressive(img, lambda done, spp: seen.append(done) and False, accum=acc, samples_per_pass=8)
        finally:
            art.set_option(None, 0)
        frames[overlap] = {"rgb": img, "acc": acc, "segments": eng.stats["segments"], "stats": eng.stats, "seen": seen}
    assert frames[2]["seen"] == [8, 16, 24] == frames[0]["seen"]
    assert frames[2]["stats"]["passes"] == frames[0]["stats"]["passes"] == 3
    assert same(frames[2], frames[0]) and same(frames[2], render(0))


def test_pixel_lists_are_not_split(gpu):
    on, off = render(2, W=36, H=24, spp=3, adaptive=True, profile=True), render(0, W=36, H=24, spp=3, adaptive=True, profile=True)
    assert on["stats"]["extend_variant"] == 3
    assert on["stats"]["passes"] == off["stats"]["passes"] and on["stats"]["extend_launches"] == off["stats"]["extend_launches"]
    assert np.array_equal(on["rgb"], off["rgb"]) and on["segments"] == off["segments"]


def test_k_paths_g_scene_is_not_split(gpu):
    on, off = render(2, scene="cow", W=48, H=32, spp=8, profile=True), render(0, scene="cow", W=48, H=32, spp=8, profile=True)
    assert on["stats"]["extend_variant"] == 4
    assert on["stats"]["passes"] == off["stats"]["passes"] == 1 and on["stats"]["extend_launches"] == 1
    assert same(on, off)


def test_auto_leaves_a_small_frame_at_one_launch(gpu):
    assert art.get_option("render.accum_overlap") == 1
    auto = render(1)
    assert auto["stats"]["passes"] == 1
    assert same(auto, render(0))


def test_profile_marks_enclose_the_path_launches(gpu):
    st = render(2, profile=True)["stats"]
    assert st["extend_launches"] == st["passes"] == 2
    assert 0 < st["extend_ms"] < st["ms"]
    assert same(render(2, profile=True), render(0))
