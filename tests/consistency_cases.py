"""Yardstick and inputs of the LR-consistency tests (tests/test_consistency_cpu.py, tests/test_consistency_gpu.py).

The yardstick is Pillow itself: ``D = Image.resize((w, h), Image.BICUBIC)`` of the output, then int64 numpy for the four integers
``sse_r, sse_g, sse_b, max_abs`` of ``e = D - L`` (include/srgd_consistency.h).  Everything is an exact integer, so every comparison
with the GPU is an equality; the three host numbers are the header's float64 formulas, written out here a second time.
``restate`` is a plain restatement of Pillow's two passes with int64 accumulators on ``oracle.pil_resample.precompute_coeffs``: it is
the only way to COUNT the accumulators that leave [0, 255] before ``clip8`` - what the "overshoot" input is built for.
Inputs: seeded random bytes, the overshoot image (0 / 255 blocks of 9 pixels: block edges fall on every phase of 4), constant
images, and ``O`` = Pillow x4 of ``L``."""
import math

import numpy as np
from PIL import Image

from oracle import pil_resample as PR

SCALE = 4
KEYS = ("lr_psnr", "lr_mse", "lr_max_abs")
TILE_W, TILE_H = 32, 15                              # LR pixels of a kernel tile (srgd_amd/csrc/consistency.hip)
# LR sizes (h, w): 5x5 - every index a border row or the single interior one; 5x37, 37x5, 6x7 - odd w: HR rows not 16-byte aligned;
# 8x8 - aligned; 16x33 - one full tile and a 1-pixel remainder tile on each axis; 31x65 - two full tiles and a 1-pixel remainder each way
SIZES = [(5, 5), (5, 37), (37, 5), (6, 7), (8, 8), (TILE_H + 1, TILE_W + 1), (2 * TILE_H + 1, 2 * TILE_W + 1)]
OVERSHOOT_SIZES = [(6, 7), (TILE_H + 1, TILE_W + 1), (2 * TILE_H + 1, 2 * TILE_W + 1)]


def random_pair(h, w, seed):
    """(O uint8 [4h,4w,3], L uint8 [h,w,3]) of seeded random bytes."""
    rng = np.random.default_rng([seed, h, w])
    return rng.integers(0, 256, (SCALE * h, SCALE * w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def overshoot_output(h, w):
    """O uint8 [4h,4w,3] of 0 / 255 blocks of 9 x 9 pixels (channel c shifted by c pixels): the edges at 9, 18, 27, 36, ... fall on
    every phase of 4, and a block is wider than the kernel's positive lobe (8 pixels), so accumulators leave [0, 255] both ways."""
    y, x = np.mgrid[0:SCALE * h, 0:SCALE * w]
    planes = [np.where(((y + c) // 9 + (x + c) // 9) % 2 == 1, 255, 0) for c in range(3)]
    return np.stack(planes, axis=2).astype(np.uint8)


def constant(h, w, value):
    return np.full((h, w, 3), value, dtype=np.uint8)


def pillow_up(lr):
    """Pillow x4 of L: the condition the sampler is given."""
    h, w, _ = lr.shape
    return np.asarray(Image.fromarray(lr, "RGB").resize((SCALE * w, SCALE * h), Image.BICUBIC))


def pillow_down(out):
    """D: Pillow's x4 reduction of O - the definition."""
    hh, ww, _ = out.shape
    assert hh % SCALE == 0 and ww % SCALE == 0
    return np.asarray(Image.fromarray(out, "RGB").resize((ww // SCALE, hh // SCALE), Image.BICUBIC))


def integers(down, lr):
    """(sse_r, sse_g, sse_b, max_abs) of e = D - L as Python ints."""
    e = down.astype(np.int64) - lr.astype(np.int64)
    sse = (e * e).sum(axis=(0, 1))
    return int(sse[0]), int(sse[1]), int(sse[2]), int(np.abs(e).max())


def record(ints, h, w):
    """The header's three float64 numbers from the four integers."""
    mse = (ints[0] + ints[1] + ints[2]) / (3 * h * w)
    return {"lr_psnr": math.inf if mse == 0 else 10.0 * math.log10(255.0 * 255.0 / mse), "lr_mse": mse, "lr_max_abs": float(ints[3])}


def yardstick(out, lr):
    """-> (D, (sse_r, sse_g, sse_b, max_abs), record) of an output and its input."""
    down = pillow_down(out)
    ints = integers(down, lr)
    return down, ints, record(ints, lr.shape[0], lr.shape[1])


def _pass(img, in_size, out_size, axis):
    """One pass of Resample.c with int64 accumulators -> (uint8 result, accumulators below 0 after the shift, above 255)."""
    bounds, kk = PR.precompute_coeffs(in_size, out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    res = np.empty((out_size,) + src.shape[1:], np.uint8)
    below = above = 0
    for xx in range(out_size):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full(src.shape[1:], 1 << (PR.PRECISION_BITS - 1), np.int64)
        for x in range(n):
            acc += src[xmin + x] * int(kk[xx, x])
        v = acc >> PR.PRECISION_BITS
        below += int((v < 0).sum())
        above += int((v > 255).sum())
        res[xx] = np.clip(v, 0, 255).astype(np.uint8)
    return np.moveaxis(res, 0, axis), below, above


def restate(out):
    """Pillow's x4 reduction restated -> (D, {"h": (below, above), "v": (below, above)}): horizontal pass over all rows, rounded to
    8 bits, then the vertical pass on that result."""
    hh, ww, _ = out.shape
    tmp, hb, ha = _pass(out, ww, ww // SCALE, axis=1)
    down, vb, va = _pass(tmp, hh, hh // SCALE, axis=0)
    return down, {"h": (hb, ha), "v": (vb, va)}
