"""Numpy restatement of the a-trous denoiser (csrc/denoise.hip, include/art.h rt_denoise): the oracle of
tests/test_gpu_denoise.py.  Every operation is an IEEE f64 + - * / or a comparison, in the order the kernels use, so
the GPU result must equal this one bit for bit.  Also the synthetic inputs and the error metric those tests share."""
import numpy as np

K = np.array([1/16, 1/4, 3/8, 1/4, 1/16]); G = np.array([1/4, 1/2, 1/4])
def taps(H, W, oy, ox):
    y0, y1 = max(0, -oy), min(H, H - oy); x0, x1 = max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1: return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
def blur3(v):
    H, W = v.shape; s = np.zeros((H, W)); sw = np.zeros((H, W))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            pq = taps(H, W, dy, dx)
            if pq is None: continue
            P, Q = pq; g = G[dy + 1] * G[dx + 1]; s[P] += g * v[Q]; sw[P] += g
    return s / sw
def atrous(c, var, alb, nrm, pos, t, iters=5, sigma_c=1.0, sigma_p=0.1, k=6, floor=0.01, demod=True):
    H, W, _ = c.shape
    a = np.maximum(alb, floor) if demod else np.ones_like(alb)
    L = c / a; q = var / (a * a); V = (q[..., 0] + q[..., 1]) + q[..., 2]
    miss = ~(t < np.inf); sp2 = sigma_p * sigma_p; sc2 = sigma_c * sigma_c
    for s in range(iters):
        step = 1 << s; Vf = blur3(V)
        sw = np.zeros((H, W)); sL = np.zeros((H, W, 3)); sV = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                pq = taps(H, W, dy * step, dx * step)
                if pq is None: continue
                P, Q = pq; h = K[dy + 2] * K[dx + 2]
                if dx == 0 and dy == 0:
                    w = np.full(sw[P].shape, h)
                else:
                    n0, n1 = nrm[P], nrm[Q]
                    dn = np.maximum((n0[..., 0]*n1[..., 0] + n0[..., 1]*n1[..., 1]) + n0[..., 2]*n1[..., 2], 0.0)
                    for _ in range(k): dn = dn * dn
                    with np.errstate(all='ignore'):
                        d = pos[Q] - pos[P]
                        dp = (n0[..., 0]*d[..., 0] + n0[..., 1]*d[..., 1]) + n0[..., 2]*d[..., 2]
                        dd = (d[..., 0]*d[..., 0] + d[..., 1]*d[..., 1]) + d[..., 2]*d[..., 2]
                        wp = np.where(dd > 0.0, np.maximum(1.0 - (dp * dp) / (sp2 * dd), 0.0), 1.0)
                    wg = np.where(miss[P] | miss[Q], np.where(miss[P] & miss[Q], 1.0, 0.0), dn * wp)
                    e = L[Q] - L[P]; dc = (e[..., 0]*e[..., 0] + e[..., 1]*e[..., 1]) + e[..., 2]*e[..., 2]
                    w = (h * wg) * (1.0 / (1.0 + dc / (sc2 * Vf[P] + 1e-12)))
                sw[P] += w; sL[P] += w[..., None] * L[Q]; sV[P] += (w * w) * V[Q]
        L = sL / sw[..., None]; V = sV / (sw * sw)
    return L * a


def denoise_reference(accum_a, accum_b, spp_each, guides, **kw):
    """rt_denoise on the CPU: the preparation (k_dn_prepare's a, b, c, var) and atrous() on a guide array (H, W, 10),
    with the library's default albedo floor (0.5, include/art.h) unless `floor` is given."""
    kw.setdefault("floor", 0.5)
    a = accum_a / float(spp_each)
    b = accum_b / float(spp_each)
    c = (a + b) / 2.0
    half = (a - b) / 2.0
    return atrous(c, half * half, guides[..., 0:3], guides[..., 3:6], guides[..., 6:9], guides[..., 9], **kw)


def write_color(color):
    """color.h:6-22 with one sample per pixel: gamma 2, clamp to [0, 0.999], 256 * x truncated (k_finalize)."""
    x = np.sqrt(1.0 * color)
    x = np.where(x < 0.0, 0.0, np.where(x > 0.999, 0.999, x))
    return (256 * x).astype(np.uint8)


def synthetic_inputs(W, H, spp_each=2, seed=0):
    """(accum_a, accum_b, guides) of a W x H frame that reaches every branch of the filter: random colour with 2 % of
    the pixels x50 outliers in one half-render, 10 % zero-albedo pixels, 20 % misses, 20 % zero-variance pixels
    (identical half-renders), a coplanar left half-image (dp is exactly 0 there), random geometry in the right one, and
    one pair of neighbouring pixels with coincident positions (dd == 0)."""
    rng = np.random.default_rng(seed)
    base = rng.random((H, W, 3))
    a = base + 0.3 * rng.random((H, W, 3))
    b = base + 0.3 * rng.random((H, W, 3))
    a[rng.random((H, W)) < 0.02] *= 50.0
    same = rng.random((H, W)) < 0.2
    b[same] = a[same]
    alb = rng.random((H, W, 3))
    alb[rng.random((H, W)) < 0.1] = 0.0
    nrm = rng.normal(size=(H, W, 3))
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    pos = rng.normal(size=(H, W, 3)) * 3.0
    yy, xx = np.mgrid[0:H, 0:W]
    left = xx < W // 2
    nrm[left] = (0.0, 0.0, 1.0)
    pos[left] = np.stack([xx * 0.125, yy * 0.125, np.zeros((H, W))], axis=2)[left]
    t = 1.0 + 9.0 * rng.random((H, W))
    miss = rng.random((H, W)) < 0.2
    if W * H >= 2:  # the coincident pair: two neighbouring hit pixels at one position
        y0, x0 = H // 2, W - 1 if W > 1 else 0
        y1, x1 = (y0, x0 - 1) if W > 1 else (y0 - 1, x0)
        miss[y0, x0] = miss[y1, x1] = False
        pos[y1, x1] = pos[y0, x0]
        nrm[y1, x1] = nrm[y0, x0]
    t[miss] = np.inf
    nrm[miss] = 0.0
    pos[miss] = np.inf
    alb[miss] = 1.0
    guides = np.ascontiguousarray(np.concatenate([alb, nrm, pos, t[..., None]], axis=2))
    return np.ascontiguousarray(a * spp_each), np.ascontiguousarray(b * spp_each), guides


def display_rmse(x, ref):
    """RMSE of sqrt(clamp(x, 0, 1)): the error of the displayed (gamma 2) frame."""
    return float(np.sqrt(np.mean((np.sqrt(np.clip(x, 0.0, 1.0)) - np.sqrt(np.clip(ref, 0.0, 1.0))) ** 2)))
