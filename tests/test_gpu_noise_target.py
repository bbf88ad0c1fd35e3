"""Noise-target rendering (rt_render_noise_target) on the GPU.  The existing renderer is the oracle: a pixel that
received n samples holds, bit for bit, the radiance sums and the RGB8 of rt_render with spp = n and the same seed; the
per-pixel counts follow the numpy restatement of the convergence test and the active-set rule (tests/nt_reference.py)."""
import functools
import json
import math
import os
import subprocess

import numpy as np
import pytest

import another_raytracer_amd as art
from another_raytracer_amd import imageio
from tests import nt_reference as nt
from tests.dn_reference import display_rmse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7
BIG = 1 << 30  # "no cap" for nt.next_active


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def world_of(scene):
    return art.scene_manager().build(scene)


def make_engine(scene, W, H, spp, seed=SEED, view=None, world=None, **kw):
    """view: (lookfrom, lookat, vfov) instead of the scene's own; world: instead of the shared one (whose compiled scene,
    renderer and workspace every engine of that scene shares)."""
    world = world or world_of(scene)
    lookfrom, lookat, vfov = view or (world.lookfrom, world.lookat, world.vfov)
    cam = art.camera(lookfrom, lookat, (0, 1, 0), vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=spp, seed=seed, **kw)
    eng.set_scene(world.objects, world.background)
    return eng


@functools.lru_cache(maxsize=None)
def uniform(scene, W, H, spp, seed=SEED, view=None):
    """rt_render at spp samples for every pixel: (rgb, acc, segments), shared by the tests and read-only."""
    eng = make_engine(scene, W, H, spp, seed, view)
    rgb = np.zeros((H, W, 3), np.uint8)
    acc = np.zeros((H, W, 3))
    eng.run(rgb, accum=acc)
    rgb.setflags(write=False)
    acc.setflags(write=False)
    return rgb, acc, eng.stats["segments"]


def noise_target(scene, W, H, cap, seed=SEED, view=None, engine_kw=None, global_scene=False, **opts):
    eng = make_engine(scene, W, H, cap, seed, view, **(engine_kw or {}))
    eng.global_scene = global_scene
    band = (opts.get("band_rows"), opts.get("band_count", 1), opts.get("band_index", 0))
    rows = len(eng.local_rows(band[0] or H, band[1], band[2]))
    out = {"rgb": np.zeros((rows, W, 3), np.uint8), "acc": np.zeros((rows, W, 3)), "count": np.zeros((rows, W), np.int32),
           "mom": np.zeros((rows, W, 2))}
    out["res"] = eng.run_noise_target(out["rgb"], accum=out["acc"], counts=out["count"], moments=out["mom"], **opts)
    out["stats"] = dict(eng.stats)
    return out


def assert_pixels_equal_uniform_renders(r, scene, W, H, view=None):
    """Every pixel with count c holds rt_render(spp = c)'s sums and RGB8."""
    for c in np.unique(r["count"]):
        rgb, acc, _ = uniform(scene, W, H, int(c), SEED, view)
        m = r["count"] == c
        assert np.array_equal(bits(r["acc"])[m], bits(acc)[m]), (scene, int(c))
        assert np.array_equal(r["rgb"][m], rgb[m]), (scene, int(c))
    assert np.array_equal(r["rgb"], nt.write_color(r["acc"], r["count"]))


# ---------------------------------------------------------------------------------------------- per-pixel equality
# rel_tol per scene and parameter set, chosen on the GPU so that at least three distinct counts each cover >= 1 % of the
# pixels; the observed histograms {count: pixels} are listed beside each value.  Scene 6 (the Cornell box) runs with
# dilation: most of its samples are black (a path that never reaches the small light returns nothing), so without it
# 93 % of the pixels retire at min_spp with four black samples and the few others mostly run to the cap.
FRAMES = {"1": (64, 36), "6": (37, 23), "7": (64, 36)}
DILATE = {"1": 0, "6": 1, "7": 0}
TOL = {
    # scene: {(min, step, cap): rel_tol}
    "1": {(4, 4, 20): 0.2,    # {4: 917, 8: 290, 12: 286, 16: 263, 20: 548}
          (2, 3, 11): 0.3,    # {2: 1341, 5: 345, 8: 260, 11: 358}
          (4, 8, 15): 0.2},   # {4: 917, 12: 561, 15: 826}
    "6": {(4, 4, 20): 0.7,    # {4: 548, 8: 15, 12: 18, 16: 26, 20: 244}   (dilated)
          (2, 3, 11): 0.7,    # {2: 667, 5: 4, 8: 13, 11: 167}
          (4, 8, 15): 0.7},   # {4: 548, 12: 24, 15: 279}
    "7": {(4, 4, 20): 0.7,    # {4: 1941, 8: 103, 12: 77, 16: 56, 20: 127}
          (2, 3, 11): 0.7,    # {2: 2078, 5: 56, 8: 41, 11: 129}
          (4, 8, 15): 0.7},   # {4: 1941, 12: 178, 15: 185}
}
TOL_6 = 0.7        # scene 6 at 37x23 without dilation, (4, 4, 20): {4: 801, 8: 9, 12: 5, 16: 9, 20: 27}
TOL_STEP70 = 0.1   # scene 1 at 37x23, (4, 70, 144): {4: 284, 74: 360, 144: 207}


def check_equality_case(scene, W, H, min_spp, step, cap, tol, dilate=0):
    r = noise_target(scene, W, H, cap, min_spp=min_spp, step_spp=step, rel_tol=tol, dilate=dilate)
    counts, pixels = np.unique(r["count"], return_counts=True)
    print(f"scene {scene} {W}x{H} (min, step, cap) = ({min_spp}, {step}, {cap}) rel_tol {tol}: "
          f"dilate {dilate} counts {dict(zip(counts.tolist(), pixels.tolist()))} rounds {r['res']['rounds']}")
    allowed = {min(min_spp + i * step, cap) for i in range(cap)}
    assert set(counts.tolist()) <= allowed
    assert (pixels >= 0.01 * W * H).sum() >= 3, "the case must exercise at least three distinct counts"
    assert_pixels_equal_uniform_renders(r, scene, W, H)
    assert r["res"]["samples"] == int(r["count"].sum()) == r["stats"]["primary"]
    assert r["res"]["rounds"] == math.ceil((int(counts.max()) - min_spp) / step)
    # without dilation a pixel retires through the test iff its final state passes it
    assert dilate or r["res"]["converged_pixels"] == int((~nt.unconverged(r["mom"][..., 0], r["mom"][..., 1], r["count"], tol)).sum())
    return r


@pytest.mark.parametrize("params", [(4, 4, 20), (2, 3, 11), (4, 8, 15)])
@pytest.mark.parametrize("scene,variant,lds_mode", [("1", 3, 3), ("6", 4, None), ("7", 4, None)])
def test_every_pixel_equals_rt_render_at_its_own_count(gpu, scene, variant, lds_mode, params):
    W, H = FRAMES[scene]
    r = check_equality_case(scene, W, H, *params, TOL[scene][params], DILATE[scene])
    # the kernel identity is the persistent kernel's: k_paths for the LDS scene, k_paths_g otherwise
    assert r["stats"]["extend_variant"] == variant
    eng = make_engine(scene, W, H, 4)
    eng.run(np.zeros((H, W, 3), np.uint8))
    for f in ("kernel_features", "kernel_textures", "kernel_lds_mode"):
        assert r["stats"][f] == eng.stats[f], f
    if lds_mode is not None:
        assert r["stats"]["kernel_lds_mode"] == lds_mode


def test_a_round_longer_than_the_accumulators_64_record_chunk(gpu):
    # step 70: every list entry's records cross the 64-record LDS chunk of k_nt_accum_list (64 + 6)
    check_equality_case("1", 37, 23, 4, 70, 144, TOL_STEP70)


@pytest.mark.parametrize("step", [63, 64, 65, 128, 130])
def test_round_lengths_around_the_chunk_size(gpu, step):
    # below, equal to and above 64 records per entry, and whole multiples: two counts suffice here
    r = noise_target("6", 37, 23, 2 + step, min_spp=2, step_spp=step, rel_tol=TOL_6)
    assert set(np.unique(r["count"]).tolist()) == {2, 2 + step}
    assert_pixels_equal_uniform_renders(r, "6", 37, 23)


# ---------------------------------------------------------------------------------------------- both extremes
# Scene 3 (two spheres with a Perlin-noise texture) seen from above, so that no pixel sees the sky: every sample's value
# follows the texture at its own jittered hit point, no two samples of a pixel are equal and every variance is positive.
# (A pixel whose samples are all equal -- the constant background, or a solid lambertian lit by it after one bounce: half
# of scene c1's pixels from the same angle -- has var == 0 and converges at any tolerance, 1e-300 included: see
# test_black_background_pixels_retire_at_min_spp.  The scenes k_paths renders all have such pixels.)
DOWN = ((13.0, 6.0, 3.0), (0.0, 0.0, 0.0), 20.0)
EXTREME = "3"


@pytest.mark.parametrize("global_scene", [False, True])
@pytest.mark.parametrize("W,H", [(37, 23), (64, 36)])
def test_a_tolerance_nothing_meets_gives_rt_render_at_the_cap(gpu, W, H, global_scene):
    cap = 12
    r = noise_target(EXTREME, W, H, cap, view=DOWN, global_scene=global_scene, min_spp=4, step_spp=4, rel_tol=1e-300)
    rgb, acc, segments = uniform(EXTREME, W, H, cap, SEED, DOWN)
    assert (r["count"] == cap).all()
    assert same_bits(r["acc"], acc) and np.array_equal(r["rgb"], rgb)
    assert r["stats"]["segments"] == segments
    assert r["stats"]["extend_variant"] == 4
    assert r["res"] == dict(r["res"], rounds=2, converged_pixels=0, samples=W * H * cap)
    assert r["stats"]["primary"] == W * H * cap and r["stats"]["passes"] == 3


@pytest.mark.parametrize("W,H", [(37, 23), (64, 36)])
def test_a_tolerance_everything_meets_gives_rt_render_at_min_spp(gpu, W, H):
    r = noise_target(EXTREME, W, H, 32, view=DOWN, min_spp=4, step_spp=4, rel_tol=1e300)
    rgb, acc, segments = uniform(EXTREME, W, H, 4, SEED, DOWN)
    assert (r["count"] == 4).all()
    assert same_bits(r["acc"], acc) and np.array_equal(r["rgb"], rgb)
    assert r["stats"]["segments"] == segments
    assert r["res"] == dict(r["res"], rounds=0, converged_pixels=W * H, samples=W * H * 4)


def test_min_spp_equal_to_the_cap_runs_no_round(gpu):
    r = noise_target("6", 37, 23, 5, min_spp=5, step_spp=3, rel_tol=1e-300)
    rgb, acc, segments = uniform("6", 37, 23, 5)
    assert (r["count"] == 5).all() and same_bits(r["acc"], acc) and np.array_equal(r["rgb"], rgb)
    assert r["res"]["rounds"] == 0 and r["stats"]["segments"] == segments


# ---------------------------------------------------------------------------------------------- round by round
@pytest.mark.parametrize("dilate", [0, 1])
def test_the_active_set_follows_the_restatement_round_by_round(gpu, dilate):
    """A run capped at min_spp + r * step_spp is the state after r rounds.  From (count_r, moments_r) the restatement
    gives A_{r+1}; the run capped one round later added exactly step_spp samples to those pixels and left every other
    pixel's sums untouched."""
    scene, (W, H), min_spp, step, tol = "6", (37, 23), 4, 3, TOL_ROUNDS
    state = [noise_target(scene, W, H, min_spp + r * step, min_spp=min_spp, step_spp=step, rel_tol=tol, dilate=dilate) for r in range(6)]
    sizes = []
    for r in range(5):
        n_r = min_spp + r * step
        a, b = state[r], state[r + 1]
        active = a["count"] == n_r  # the pixels round r traced (r = 0: every pixel)
        nxt = nt.next_active(active, n_r, a["mom"], BIG, rel_tol=tol, dilate=bool(dilate))
        sizes.append(int(nxt.sum()))
        assert np.array_equal(b["count"], a["count"] + step * nxt.astype(np.int32)), (r, dilate)
        for key in ("acc", "mom"):
            assert np.array_equal(bits(a[key])[~nxt], bits(b[key])[~nxt]), (r, key)
        assert b["res"]["rounds"] == (r + 1 if nxt.any() else a["res"]["rounds"])
        assert_pixels_equal_uniform_renders(b, scene, W, H)
    print(f"dilate {dilate}: active pixels per round {sizes}")
    assert any(s % 64 for s in sizes) and sizes[0] > sizes[-1] > 0
    if dilate:
        plain = noise_target(scene, W, H, min_spp + 5 * step, min_spp=min_spp, step_spp=step, rel_tol=tol)
        assert (state[5]["count"] >= plain["count"]).all() and (state[5]["count"] > plain["count"]).any()


TOL_ROUNDS = 0.7  # scene 6 at 37x23, (min, step) = (4, 3): active pixels per round [851, 50, 41, 39, 33, 27], dilated [851, 303, 281, 271, 253, 238]


# ---------------------------------------------------------------------------------------------- moments
def prefix_sums(scene, W, H, n):
    """The running radiance sums after 1 .. n samples (rt_render_progressive, one sample per pass)."""
    eng = make_engine(scene, W, H, n)
    rgb = np.zeros((H, W, 3), np.uint8)
    acc = np.zeros((H, W, 3))
    snaps = []
    eng.run_progressive(rgb, lambda done, spp: snaps.append(acc.copy()) and False, accum=acc, samples_per_pass=1)
    assert len(snaps) == n
    return snaps


def test_the_moments_are_the_sums_of_the_samples_luminances(gpu):
    """S1 = sum y_j, S2 = sum y_j^2 over the pixel's samples.  The samples are recovered as differences of consecutive
    running sums, d_j = fl(A_j - A_{j-1}) with A_j = fl(A_{j-1} + x_j), so with u = 2^-53 and radiance >= 0 (the sums grow
    monotonically to the final A):  |A_j - (A_{j-1} + x_j)| <= u A  and  |d_j - (A_j - A_{j-1})| <= u d_j <= u A, hence
    |d_j - x_j| <= 2 u A per channel and, with L = lum(A) (>= S1 up to rounding, >= every y_j),
        |y(d_j) - y_j| <= 2 u L + 4 u y_j          (3 products and 2 sums round on either side),
        |S1' - S1|    <= sum_j (2 u L + 4 u y_j) + 2 (n - 1) u S1 <= (4 n + 4) u L,
        |S2' - S2|    <= sum_j 2 y_j (2 u L + 4 u y_j) + 2 u S2 + 2 (n - 1) u S2 <= (2 n + 12) u L^2   (S2 <= L^2),
    to first order in u; the bounds below add 4 to each factor for the second-order terms."""
    scene, (W, H), n = "6", (37, 23), 11
    snaps = prefix_sums(scene, W, H, n)
    u = 2.0 ** -53
    for opts in (dict(min_spp=n), dict(min_spp=2, step_spp=3, rel_tol=1e-300)):  # the base-pass and the list-mode accumulators
        r = noise_target(scene, W, H, n, **opts)
        assert set(np.unique(r["count"]).tolist()) <= {2, 5, 8, 11}
        s1 = np.zeros((H, W))
        s2 = np.zeros((H, W))
        final = np.zeros((H, W, 3))
        prev = np.zeros((H, W, 3))
        for j in range(n):
            live = r["count"] > j
            y = nt.luminance(snaps[j] - prev)
            s1 += np.where(live, y, 0.0)
            s2 += np.where(live, y * y, 0.0)
            final = np.where(live[..., None], snaps[j], final)
            prev = snaps[j]
        assert same_bits(final, r["acc"])
        L = np.maximum(nt.luminance(final), r["mom"][..., 0])
        cnt = r["count"].astype(np.float64)
        assert (np.abs(s1 - r["mom"][..., 0]) <= (4 * cnt + 8) * u * L).all()
        assert (np.abs(s2 - r["mom"][..., 1]) <= (2 * cnt + 16) * u * L * L).all()
        assert (r["mom"][..., 0] > 0).any()


def test_black_background_pixels_retire_at_min_spp(gpu):
    # scene 6's background is black: a pixel whose every sample leaves the box unlit sums zeros, var == 0 exactly, and
    # it retires at min_spp whatever the tolerance
    W, H, cap = 64, 36, 12
    r = noise_target("6", W, H, cap, min_spp=4, step_spp=4, rel_tol=1e-300)
    _, acc, _ = uniform("6", W, H, cap)
    black = (acc == 0).all(axis=2)
    assert black.sum() >= 0.01 * W * H
    assert (r["count"][black] == 4).all() and (r["mom"][black] == 0).all() and (r["rgb"][black] == 0).all()
    assert_pixels_equal_uniform_renders(r, "6", W, H)
    assert r["res"]["converged_pixels"] == int((~nt.unconverged(r["mom"][..., 0], r["mom"][..., 1], r["count"], 1e-300)).sum())
    assert r["res"]["converged_pixels"] >= int((r["count"] < cap).sum()) >= black.sum()


# ---------------------------------------------------------------------------------------------- independence
IND = dict(min_spp=4, step_spp=4)


@functools.lru_cache(maxsize=None)
def whole_frame():
    r = noise_target("6", 37, 23, 20, rel_tol=TOL_6, **IND)
    for k in ("rgb", "acc", "count", "mom"):
        r[k].setflags(write=False)
    return r


@pytest.mark.parametrize("band_rows,band_count", [(1, 2), (1, 3), (5, 2), (5, 3)])
def test_band_renders_unite_to_the_whole_frame(gpu, band_rows, band_count):
    W, H = 37, 23
    whole = whole_frame()
    tol = TOL_6
    seen = np.zeros(H, bool)
    for b in range(band_count):
        rows = make_engine("6", W, H, 20).local_rows(band_rows, band_count, b)
        r = noise_target("6", W, H, 20, rel_tol=tol, band_rows=band_rows, band_count=band_count, band_index=b, **IND)
        assert same_bits(r["acc"], whole["acc"][rows]) and same_bits(r["mom"], whole["mom"][rows])
        assert np.array_equal(r["count"], whole["count"][rows]) and np.array_equal(r["rgb"], whole["rgb"][rows])
        assert r["stats"]["local_rows"] == len(rows)
        seen[rows] = True
    assert seen.all()


def test_pass_size_scene_placement_and_repetition_do_not_change_a_bit(gpu):
    W, H = 37, 23
    whole = whole_frame()
    tol = TOL_6

    def same(r):
        return (same_bits(r["acc"], whole["acc"]) and same_bits(r["mom"], whole["mom"]) and np.array_equal(r["count"], whole["count"])
                and np.array_equal(r["rgb"], whole["rgb"]) and r["stats"]["segments"] == whole["stats"]["segments"] and r["res"]["rounds"] == whole["res"]["rounds"]
                and r["res"]["converged_pixels"] == whole["res"]["converged_pixels"])

    assert same(noise_target("6", W, H, 20, rel_tol=tol, **IND))  # an identical call
    assert whole["stats"]["passes"] == 1 + whole["res"]["rounds"]
    for spp_pass in (1, 3, 7):  # the base pass in 4, 2 and 1 passes
        r = noise_target("6", W, H, 20, rel_tol=tol, engine_kw=dict(samples_per_pass=spp_pass), **IND)
        assert same(r), spp_pass
        assert r["stats"]["passes"] == math.ceil(4 / spp_pass) + whole["res"]["rounds"]
    # a round whose slots exceed the pass workspace splits into sub-passes by sample range: with one sample per pass the
    # workspace holds 960 slots (the 37x23 frame's 8x8 tiles), and the dilated first round has 303 pixels x 4 samples
    wide = noise_target("6", W, H, 20, rel_tol=tol, dilate=1, **IND)
    split = noise_target("6", W, H, 20, rel_tol=tol, dilate=1, engine_kw=dict(samples_per_pass=1), **IND)
    assert same_bits(split["acc"], wide["acc"]) and same_bits(split["mom"], wide["mom"]) and np.array_equal(split["count"], wide["count"])
    assert split["stats"]["segments"] == wide["stats"]["segments"] and split["res"] == dict(wide["res"], ms=split["res"]["ms"])
    assert split["stats"]["passes"] > 4 + wide["res"]["rounds"]
    assert same(noise_target("6", W, H, 20, rel_tol=tol, profile=True, **IND))
    # the LDS-scene kernel and the HBM-scene kernel trace the same paths
    a = noise_target("1", 64, 36, 20, rel_tol=TOL["1"][(4, 4, 20)], **IND)
    b = noise_target("1", 64, 36, 20, rel_tol=TOL["1"][(4, 4, 20)], global_scene=True, **IND)
    assert a["stats"]["extend_variant"] == 3 and b["stats"]["extend_variant"] == 4
    assert same_bits(a["acc"], b["acc"]) and same_bits(a["mom"], b["mom"]) and np.array_equal(a["count"], b["count"])
    assert a["stats"]["segments"] == b["stats"]["segments"]


def test_device_buffers_give_the_same_bits(gpu):
    import torch
    W, H = 37, 23
    whole = whole_frame()
    eng = make_engine("6", W, H, 20)
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
    count = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    mom = torch.zeros((H, W, 2), dtype=torch.float64, device="cuda")
    res = eng.run_noise_target(rgb, accum=acc, counts=count, moments=mom, rel_tol=TOL_6, **IND)
    assert same_bits(acc.cpu().numpy(), whole["acc"]) and same_bits(mom.cpu().numpy(), whole["mom"])
    assert np.array_equal(count.cpu().numpy(), whole["count"]) and np.array_equal(rgb.cpu().numpy(), whole["rgb"])
    assert res["rounds"] == whole["res"]["rounds"]
    with pytest.raises(ValueError):
        eng.run_noise_target(rgb, accum=np.zeros((H, W, 3)), **IND)  # host and device buffers mixed
    only_rgb = np.zeros((H, W, 3), np.uint8)
    eng.run_noise_target(only_rgb, rel_tol=TOL_6, **IND)  # every optional buffer left out
    assert np.array_equal(only_rgb, whole["rgb"])


def test_a_refused_workspace_fails_cleanly(gpu, options):
    W, H = 64, 36
    # a scene of its own: its renderer has no workspace yet, so the first call must allocate
    eng = make_engine("6", W, H, 12, world=art.scene_manager().build("6"))
    rgb = np.zeros((H, W, 3), np.uint8)
    options("test.fault_workspace_bytes", 4096)
    with pytest.raises(art.RTError) as e:
        eng.run_noise_target(rgb, min_spp=4, step_spp=4, rel_tol=0.2)
    assert e.value.code == -3 and "test.fault_workspace_bytes" in str(e.value)
    options("test.fault_workspace_bytes", 0)
    res = eng.run_noise_target(rgb, min_spp=4, step_spp=4, rel_tol=0.2)  # the next call allocates again
    want = noise_target("6", W, H, 12, min_spp=4, step_spp=4, rel_tol=0.2)
    assert np.array_equal(rgb, want["rgb"]) and res["samples"] == want["res"]["samples"]


def test_art_render_noise_target_writes_the_frame_and_its_json_line(gpu, tmp_path):
    W, H, cap = 64, 48, 32
    png = tmp_path / "out.png"
    exe = os.path.join(ROOT, "another_raytracer_amd", "art_render")
    out = subprocess.run([exe, "6", str(W), str(H), str(cap), str(png), "--noise-target", "0.1", "--min-spp", "4", "--step-spp", "4", "--seed", str(SEED)],  # (art_render dilates)
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    line, summary = [json.loads(x) for x in out.stdout.strip().splitlines()]
    r = noise_target("6", W, H, cap, min_spp=4, step_spp=4, rel_tol=0.1, dilate=1)
    assert np.array_equal(imageio.load_image(str(png)), r["rgb"])
    assert line["noise_target"] == 0.1 and line["rounds"] == r["res"]["rounds"] and line["ms"] > 0
    assert line["mean_spp"] == pytest.approx(r["count"].mean(), rel=1e-5)
    assert line["converged_share"] == pytest.approx(r["res"]["converged_pixels"] / (W * H), rel=1e-5)
    assert summary["segments"] == r["stats"]["segments"]


# ---------------------------------------------------------------------------------------------- benefit
BW, BH, BCAP = 160, 90, 256


def benefit_table(scene="6", seeds=(1, 2, 3, 4, 5), rel_tol=0.05, **opts):
    """Per seed: display RMSE against a 1024-spp render of the noise-target frame (defaults, cap 256) and of a uniform
    rt_render at ceil(mean count) samples (the rounding favours the uniform render)."""
    ref = uniform(scene, BW, BH, 1024, 99)[1] / 1024.0
    rows = []
    for seed in seeds:
        r = noise_target(scene, BW, BH, BCAP, seed=seed, rel_tol=rel_tol, **opts)
        mean = float(r["count"].mean())
        spp = math.ceil(mean)
        _, acc, _ = uniform(scene, BW, BH, spp, seed)
        e_nt = display_rmse(r["acc"] / r["count"][..., None], ref)
        e_un = display_rmse(acc / spp, ref)
        rows.append(dict(seed=seed, mean_spp=mean, uniform_spp=spp, rounds=r["res"]["rounds"], rmse_noise_target=e_nt, rmse_uniform=e_un, ratio=e_nt / e_un))
    return rows


def test_noise_target_beats_the_uniform_render_at_equal_samples(gpu):
    """Scene 6 at 160x90, cap 256, defaults (min 32, step 32, rel_tol 0.05), seeds 1..5, ratio = noise-target RMSE / uniform
    RMSE.  Measured on an MI355X:
        dilate 1: mean spp 145.0 .. 146.8, ratio 0.778 0.783 0.755 0.780 0.768 (mean 0.773, std 0.012): asserted, per seed;
        dilate 0: mean spp  94.1 ..  95.4, ratio 1.230 1.225 1.212 1.237 1.205 (mean 1.222, std 0.013): the noise-target
                  frame is WORSE.  Most of this scene's samples are black, so a pixel whose first 32 samples are all black
                  has var == 0 and retires although it is among the noisiest; dilation keeps it active beside a lit
                  neighbour.  Printed, not asserted (DESIGN.md section 4.6 has the table for scenes 1 and 8 too)."""
    for dilate in (1, 0):
        rows = benefit_table("6", dilate=dilate)
        for x in rows:
            print(f"dilate {dilate}", json.dumps(x))
        if dilate:
            assert all(x["rmse_noise_target"] < x["rmse_uniform"] for x in rows), rows
