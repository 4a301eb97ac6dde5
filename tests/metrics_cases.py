"""The yardstick of the metrics tests: Y-channel PSNR, RGB PSNR and Y-channel SSIM with a border crop, restated in float64 numpy
LITERALLY from the definition in include/srgd_metrics.h - the 2-D 121-tap Gaussian window as an explicit double loop over the valid
positions, not the separable form the kernels compute.  Test infrastructure only: product code never imports it.

Tolerances of the GPU tests (both sides accumulate in float64 and differ in summation order and in separable against 2-D
filtering only): at the test shapes (<= 1.5e5 pixels, values <= 255^2 = 65,025) a filtered second moment carries at most about
121 * 2^-53 * 65,025 ~ 1e-9 absolute error against C2 = 58.5, a mean squared error at most about 1.5e5 * 2^-53 relative error:
|ssim - ssim_ref| <= 1e-9, |psnr - psnr_ref| <= 1e-9 dB for finite values, inf and NaN compared by kind."""
import functools
import math

import numpy as np

KEYS = ("psnr_y", "psnr_rgb", "ssim_y")
TOL = 1e-9
TILE_H, TILE_W = 8, 32                  # SSIM positions per workgroup of the kernels: the shapes below straddle their edges
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def edge_shapes(crop):
    """(h, w) one pixel below, at and above the second tile edge in each dimension after crop and the 10-pixel window margin."""
    return [(2 * TILE_H + 10 + 2 * crop + d, 2 * TILE_W + 10 + 2 * crop + d) for d in (-1, 0, 1)]


def window():
    g = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) ** 2) / 4.5)
    g = g / g.sum()
    return np.outer(g, g)


def quantise(out01):
    """[3,h,w] float32 in [0,1] -> [h,w,3] int64: the fp32 product with 255 and truncation (what the image is saved as)."""
    out01 = np.asarray(out01, dtype=np.float32)
    return (out01 * np.float32(255.0)).astype(np.int64).transpose(1, 2, 0)


def luma(rgb):
    """[h,w,3] integer levels -> [h,w] float64 BT.601 luma (MATLAB rgb2ycbcr), not rounded."""
    rgb = rgb.astype(np.float64)
    return 65.481 * (rgb[..., 0] / 255.0) + 128.553 * (rgb[..., 1] / 255.0) + 24.966 * (rgb[..., 2] / 255.0) + 16.0


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return math.inf if mse == 0.0 else float(10.0 * np.log10(255.0 ** 2 / mse))


def ssim_literal(x, y):
    """Mean of the SSIM map of two float64 [h,w] images over the (h-10) x (w-10) valid positions, 2-D window, double loop."""
    win = window()
    vh, vw = x.shape[0] - 10, x.shape[1] - 10
    stack = np.stack([x, y, x * x, y * y, x * y])
    vals = np.empty((vh, vw))
    for i in range(vh):
        for j in range(vw):
            mx, my, exx, eyy, exy = (stack[:, i:i + 11, j:j + 11] * win).sum(axis=(1, 2))
            sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
            vals[i, j] = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return float(vals.mean())


def ssim_separable(x, y):
    """The same mean with the window applied separably (along x, then along y): the form the kernels compute."""
    g = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) ** 2) / 4.5)
    g = g / g.sum()
    vh, vw = x.shape[0] - 10, x.shape[1] - 10

    def filt(a):
        hx = sum(g[k] * a[:, k:k + vw] for k in range(11))
        return sum(g[k] * hx[k:k + vh, :] for k in range(11))
    mx, my, exx, eyy, exy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    return float((((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))).mean())


def restate_u8(q, ref_u8, crop, ssim=ssim_literal):
    """The three numbers of two [h,w,3] images of integer levels (``q``: the quantised output or a decoded PNG)."""
    h, w = q.shape[:2]
    assert ref_u8.shape == q.shape and h - 2 * crop >= 11 and w - 2 * crop >= 11
    q, r = (a[crop:h - crop, crop:w - crop].astype(np.int64) for a in (q, ref_u8))
    yo, yr = luma(q), luma(r)
    return {"psnr_y": psnr(yo, yr), "psnr_rgb": psnr(q, r), "ssim_y": ssim(yo, yr)}


def restate(out01, ref_u8, crop, ssim=ssim_literal):
    """``restate_u8`` of the quantised [3,h,w] float32 output; a non-finite value inside the crop makes all three NaN."""
    out01 = np.asarray(out01, dtype=np.float32)
    h, w = out01.shape[1:]
    if not np.isfinite(out01[:, crop:h - crop, crop:w - crop]).all():
        return {k: math.nan for k in KEYS}
    return restate_u8(quantise(np.where(np.isfinite(out01), out01, np.float32(0))), ref_u8, crop, ssim)


def pair(h, w, seed):
    """A seeded (out01 [3,h,w] float32 in [0,1), ref_u8 [h,w,3] uint8) pair of unrelated random images."""
    rng = np.random.default_rng(seed)
    return rng.random((3, h, w), dtype=np.float32), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def noisy_pair(h, w, seed):
    """The realistic high-SSIM regime, where the variance terms cancel: a smooth output and ref = quantised output +- 0..3."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([0.5 + 0.4 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0 - c) for c in range(3)]).astype(np.float32)
    out01 = np.clip(base + rng.normal(0, 0.02, base.shape).astype(np.float32), 0, 1).astype(np.float32)
    ref = np.clip(quantise(out01) + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
    return out01, ref


@functools.lru_cache(maxsize=None)
def case(kind, h, w, crop, seed):
    """(out01, ref_u8, restatement) of a seeded case, computed once per session and shared; treat the arrays as read-only."""
    out01, ref = (pair if kind == "random" else noisy_pair)(h, w, seed)
    return out01, ref, restate(out01, ref, crop)


def same_kind_or_close(got, want, tol=TOL):
    """inf and NaN by kind, finite values within ``tol``."""
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= tol
