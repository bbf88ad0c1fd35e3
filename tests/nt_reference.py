"""numpy restatement of noise-target rendering's per-pixel rules (csrc/noise_target.hip, include/art.h
rt_render_noise_target): the convergence test, the active-set rule with and without dilation, and write_color with a
per-pixel sample count.  Every step is one IEEE f64 operation in the kernel's order (numpy neither contracts nor
reassociates), so the results equal the GPU's bit for bit."""
import numpy as np

LUMA = (0.2126, 0.7152, 0.0722)


def luminance(rgb):
    """y = (0.2126*r + 0.7152*g) + 0.0722*b of radiance records (..., 3)."""
    rgb = np.asarray(rgb, np.float64)
    return (LUMA[0] * rgb[..., 0] + LUMA[1] * rgb[..., 1]) + LUMA[2] * rgb[..., 2]


def unconverged(s1, s2, n, rel_tol=0.05, lum_floor=0.01):
    """True where the mean of n samples with luminance sums s1, s2 is not yet within the tolerance (nt_unconverged).
    n: an int or an integer array of the sums' shape, >= 2."""
    s1 = np.asarray(s1, np.float64)
    s2 = np.asarray(s2, np.float64)
    dn = np.asarray(n).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        mean = s1 / dn
        var = (s2 - s1 * mean) / (dn - 1.0)
        var = np.where(var < 0.0, 0.0, var)
        se2 = var / dn
        thr = np.float64(rel_tol) * (mean + np.float64(lum_floor))
        return ~(se2 <= thr * thr)


def dilate3(flag):
    """OR of a 2-D boolean plane over every pixel's 3x3 neighbourhood, clipped at the image border."""
    flag = np.asarray(flag, bool)
    h, w = flag.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = flag
    out = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            out |= pad[dy:dy + h, dx:dx + w]
    return out


def next_active(active, n_done, moments, cap, rel_tol=0.05, lum_floor=0.01, dilate=False):
    """A_{r+1} from A_r (2-D bool), the common sample count n_done of the active pixels and the moments (H, W, 2) after
    round r: active, below the cap, and unconverged -- with dilate, some active pixel of the 3x3 neighbourhood (the pixel
    itself included) unconverged."""
    active = np.asarray(active, bool)
    unc = active & unconverged(moments[..., 0], moments[..., 1], n_done, rel_tol, lum_floor)
    want = dilate3(unc) if dilate else unc
    return active & want & (n_done < cap)


def write_color(acc, count):
    """color.h:6-22 with every pixel's own count: sqrt(acc * (1.0 / count)), clamp to [0, 0.999], 256 * x truncated
    (k_nt_finalize; k_finalize's arithmetic)."""
    scale = 1.0 / np.asarray(count).astype(np.float64)
    x = np.sqrt(scale[..., None] * np.asarray(acc, np.float64))
    x = np.where(x < 0.0, 0.0, np.where(x > 0.999, 0.999, x))
    return (256 * x).astype(np.uint8)
