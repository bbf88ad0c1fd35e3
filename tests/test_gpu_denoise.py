"""The a-trous denoiser (rt_denoise, rt_render_denoised): bit equality with the numpy restatement (tests/dn_reference.py)
on synthetic and rendered inputs, the one-call path against the same steps through the public calls, a clean failure
when the workspace cannot grow, and the quality inequality: the denoised frame is closer to a 1024-spp render than the
noisy one."""
import functools

import numpy as np
import pytest

import another_raytracer_amd as art
from tests.dn_reference import denoise_reference, display_rmse, synthetic_inputs, write_color

pytestmark = pytest.mark.gpu


def assert_same_bits(got, want, what):
    bad = np.flatnonzero(got.view(np.int64).ravel() != want.view(np.int64).ravel())
    if len(bad):
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ; first at flat index {i}: gpu {got.ravel()[i]!r} "
                             f"({got.view(np.int64).ravel()[i]:#x}) reference {want.ravel()[i]!r} ({want.view(np.int64).ravel()[i]:#x})")


def make_engine(scene, W, H, spp, seed):
    world = art.scene_manager().build(scene)
    cam = art.camera(world.lookfrom, world.lookat, (0, 1, 0), world.vfov, W / H, world.aperture, 10.0, 0.0, 1.0)
    eng = art.engine(cam, art.engine_mode.single, width=W, height=H, samples_per_pixel=spp, seed=seed)
    eng.set_scene(world.objects, world.background)
    return eng


def render_accum(scene, W, H, spp, seed):
    eng = make_engine(scene, W, H, spp, seed)
    rgb = np.zeros((H, W, 3), np.uint8)
    acc = np.zeros((H, W, 3))
    eng.run(rgb, accum=acc)
    return acc


# ---------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("W,H,iters", [(37, 23, 5), (1, 1, 5), (5, 1, 3), (2, 70, 5), (64, 36, 1), (33, 40, 5)])
def test_filter_equals_the_numpy_restatement_bit_for_bit(gpu, options, W, H, iters):
    a, b, guides = synthetic_inputs(W, H, spp_each=2, seed=W * 1000 + H)
    want = denoise_reference(a, b, 2, guides, iters=iters)
    # the default kernels (tap spacings 1 and 2 from an LDS tile), the direct-load kernels alone, and the mix
    for lds_iterations in (2, 0, 1):
        options("denoise.lds_iterations", lds_iterations)
        rgb = np.zeros((H, W, 3), np.uint8)
        out, ms = art.denoise(a, b, 2, guides, out_rgb8=rgb, iterations=iters)
        assert_same_bits(out, want, f"{W}x{H}x{iters}, denoise.lds_iterations {lds_iterations}")
        assert np.array_equal(rgb, write_color(out))
        assert ms >= 0.0


def test_filter_options_reach_the_kernels(gpu):
    W, H = 37, 23
    a, b, guides = synthetic_inputs(W, H, spp_each=3, seed=5)
    out, _ = art.denoise(a, b, 3, guides, iterations=2, normal_squarings=3, sigma_color=2.5, sigma_plane=0.3, albedo_floor=0.05)
    want = denoise_reference(a, b, 3, guides, iters=2, k=3, sigma_c=2.5, sigma_p=0.3, floor=0.05)
    assert_same_bits(out, want, "options")


def test_no_demodulate_matches_demod_false(gpu):
    W, H = 37, 23
    a, b, guides = synthetic_inputs(W, H, seed=6)
    out, _ = art.denoise(a, b, 2, guides, demodulate=False)
    assert_same_bits(out, denoise_reference(a, b, 2, guides, demod=False), "no demodulation")
    with_demod, _ = art.denoise(a, b, 2, guides)
    assert not np.array_equal(out, with_demod)


def test_device_buffers_give_the_same_bits(gpu):
    import torch
    W, H = 33, 40
    a, b, guides = synthetic_inputs(W, H, seed=7)
    rgb = np.zeros((H, W, 3), np.uint8)
    out, _ = art.denoise(a, b, 2, guides, out_rgb8=rgb)
    d_rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    d_out, _ = art.denoise(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 2, torch.from_numpy(guides).cuda(), out_rgb8=d_rgb)
    assert d_out.device.type == "cuda"
    assert_same_bits(d_out.cpu().numpy(), out, "device buffers")
    assert np.array_equal(d_rgb.cpu().numpy(), rgb)


@functools.lru_cache(maxsize=None)
def cornell_inputs():
    """Scene 6 at 96x64: two 2-spp half-renders (seeds 1, 2) and the GPU guides."""
    W, H = 96, 64
    a = render_accum("6", W, H, 2, 1)
    b = render_accum("6", W, H, 2, 2)
    guides = make_engine("6", W, H, 2, 1).render_guides()
    for x in (a, b, guides):
        x.setflags(write=False)
    return a, b, guides


def test_rendered_inputs_equal_the_numpy_restatement(gpu):
    a, b, guides = cornell_inputs()
    rgb = np.zeros((64, 96, 3), np.uint8)
    out, _ = art.denoise(a, b, 2, guides, out_rgb8=rgb)
    assert_same_bits(out, denoise_reference(a, b, 2, guides), "scene 6")
    assert np.array_equal(rgb, write_color(out))
    assert np.isfinite(out).all() and not np.array_equal(out, (a + b) / 4.0)


def test_one_call_path_equals_the_steps_made_by_hand(gpu):
    W, H = 96, 64
    a, b, guides = cornell_inputs()
    rgb = np.zeros((H, W, 3), np.uint8)
    out, _ = art.denoise(a, b, 2, guides, out_rgb8=rgb, iterations=4, sigma_color=1.5)
    eng = make_engine("6", W, H, 4, 1)  # 4 spp: two half-renders of 2 spp, seeds 1 and 2
    one_rgb = np.zeros((H, W, 3), np.uint8)
    one = np.zeros((H, W, 3))
    ms = eng.run_denoised(one_rgb, color=one, iterations=4, sigma_color=1.5)
    assert_same_bits(one, out, "rt_render_denoised")
    assert np.array_equal(one_rgb, rgb)
    assert ms >= 0 and eng.stats["primary"] == W * H * 4 and eng.stats["segments"] > eng.stats["primary"]
    # and with everything on the device
    import torch
    d_rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    d_one = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda")
    eng.run_denoised(d_rgb, color=d_one, iterations=4, sigma_color=1.5)
    assert_same_bits(d_one.cpu().numpy(), out, "rt_render_denoised, device buffers")
    assert np.array_equal(d_rgb.cpu().numpy(), rgb)


def test_a_refused_workspace_fails_cleanly(gpu, options):
    W, H = 64, 36
    a, b, guides = synthetic_inputs(W, H, seed=8)
    want, _ = art.denoise(a, b, 2, guides)
    bigger = synthetic_inputs(4 * W, 4 * H, seed=9)  # larger than any frame these tests denoise: the workspace must grow
    options("test.fault_workspace_bytes", 4096)
    with pytest.raises(art.RTError) as e:
        art.denoise(bigger[0], bigger[1], 2, bigger[2])
    assert e.value.code == -3 and "test.fault_workspace_bytes" in str(e.value)
    options("test.fault_workspace_bytes", 0)
    again, _ = art.denoise(a, b, 2, guides)  # the workspace was released: the next call allocates again
    assert_same_bits(again, want, "after the refused growth")


# ---------------------------------------------------------------------------------------------- quality
QW, QH = 160, 90


@functools.lru_cache(maxsize=None)
def quality_reference(scene):
    ref = render_accum(scene, QW, QH, 1024, 99) / 1024.0
    guides = make_engine(scene, QW, QH, 2, 1).render_guides()
    ref.setflags(write=False)
    guides.setflags(write=False)
    return ref, guides


@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("spp", [4, 16])
@pytest.mark.parametrize("scene", ["1", "6"])
def test_denoised_frame_is_closer_to_the_converged_render(gpu, scene, spp, demodulate):
    ref, guides = quality_reference(scene)
    half = spp // 2
    a = render_accum(scene, QW, QH, half, 1)
    b = render_accum(scene, QW, QH, half, 2)
    noisy = (a + b) / float(spp)
    out, _ = art.denoise(a, b, half, guides, demodulate=demodulate)
    e_noisy, e_dn = display_rmse(noisy, ref), display_rmse(out, ref)
    print(f"scene {scene} {spp} spp demodulate={demodulate}: noisy {e_noisy:.5f} denoised {e_dn:.5f} ratio {e_dn / e_noisy:.3f}")
    assert e_dn < e_noisy, (scene, spp, demodulate, e_dn / e_noisy)
