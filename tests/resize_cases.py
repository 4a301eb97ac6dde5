"""Numpy integer restatement of ``PIL.Image.resize`` of an 8-bit RGB image for the three filters of include/srgd_resize.h, and the
case tables the CPU and the GPU tests of srgd_amd.resize share.

The algorithm is Pillow's ``src/libImaging/Resample.c`` (Pillow 12): ``precompute_coeffs`` (double weights of the window clipped to
the image, summed left to right and renormalised), ``normalize_coeffs_8bpc`` (22-bit fixed point, round half away from zero),
``ImagingResampleHorizontal_8bpc`` over all input rows, rounded to 8 bits (accumulator ``1 << 21``, ``clip8(acc >> 22)``), then
``ImagingResampleVertical_8bpc`` on that result; a pass whose in == out is skipped.  tests/test_resize_cpu.py pins it against Pillow
itself on every case, filter and pattern below; the GPU tests compare the kernels with it and never import Pillow's resize."""
from __future__ import annotations

import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
FILTERS = {"bicubic": 3, "bilinear": 2, "lanczos": 1}         # name -> PIL.Image.Resampling number = the library's
SUPPORT = {"bicubic": 2.0, "bilinear": 1.0, "lanczos": 3.0}
MAX_RATIO = 8
H_TILE = (32, 16)                                            # horizontal kernel: output pixels x rows of a tile
V_TILE = (256, 16)                                           # vertical kernel: bytes x output rows of a tile


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


WEIGHT = {"bicubic": _bicubic, "bilinear": _bilinear, "lanczos": _lanczos}


def ksize(in_size, out_size, filter):
    filterscale = max(in_size / out_size, 1.0)
    return int(math.ceil(SUPPORT[filter] * filterscale)) * 2 + 1


@functools.lru_cache(maxsize=None)
def table(in_size, out_size, filter):
    """-> (bounds [out,2] int32 = (xmin, count), coeffs [out, ksize] int32 fixed point, zero from count on)."""
    weight = WEIGHT[filter]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = SUPPORT[filter] * filterscale
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ks), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)               # C cast: truncation toward zero
        count = min(int(center + support + 0.5), in_size) - xmin
        w = [weight((x + xmin - center + 0.5) * ss) for x in range(count)]
        ww = 0.0
        for v in w:                                              # left to right, like the C loop
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, count)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


def _pass(img, bounds, kk, axis):
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.uint8)
    for xx in range(bounds.shape[0]):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for x in range(n):
            acc += src[xmin + x] * int(kk[xx, x])
        assert np.abs(acc).max() < 2 ** 31                       # Pillow's accumulator is an int32
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_u8(img_hwc, out_h, out_w, filter):
    """uint8 [H,W,3] -> uint8 [out_h,out_w,3]: ``Image.resize((out_w, out_h), FILTER)`` bit for bit."""
    h, w, _ = img_hwc.shape
    tmp = _pass(img_hwc, *table(w, out_w, filter), axis=1) if out_w != w else img_hwc        # horizontal first
    return _pass(tmp, *table(h, out_h, filter), axis=0) if out_h != h else tmp.copy()


# ((h_in, w_in), (h_out, w_out))
CASES = [
    # windows clipped at both ends at once; one-pixel outputs; one-row images
    ((5, 7), (3, 2)), ((16, 16), (1, 1)), ((8, 8), (1, 1)), ((1, 9), (1, 3)), ((3, 200), (2, 25)),
    # ratio 1:8 up: every window clipped
    ((1, 1), (8, 8)), ((8, 6), (64, 48)),
    # ratio 8:1 down: 49 lanczos taps, the table's full width
    ((64, 48), (8, 6)),
    # non-integer ratios, down on one axis and up on the other, widths that are no multiples of 4
    ((37, 23), (23, 37)), ((129, 67), (43, 100)),
    # one pass skipped - the horizontal one, then the vertical one
    ((33, 65), (33, 31)), ((65, 33), (31, 33)),
    # what --outscale 2 and --outscale 3 do to a 10x13 input
    ((40, 52), (20, 26)), ((40, 52), (30, 39)),
    # the horizontal kernel's tile of 32 output pixels x 16 rows and the vertical kernel's 16 output rows: tile - 1, tile, tile + 1
    ((17, 40), (15, 31)), ((15, 45), (16, 32)), ((16, 50), (17, 33)),
    # the vertical kernel's tile of 256 bytes: 255 bytes, 258 bytes (85 and 86 pixels); 256 bytes is no multiple of 3, 264 is a
    # dword-aligned row that ends 8 bytes into its second tile
    ((9, 100), (9, 85)), ((9, 100), (12, 86)), ((12, 64), (9, 88)),
    # both passes skipped: the copy, on the dword path and on the byte path
    ((6, 8), (6, 8)), ((5, 7), (5, 7)),
]
SMALLEST = ((5, 7), (3, 2))


def in_range(in_size, out_size):
    """Whether the library takes the case: per axis a ratio of at most 8 either way.  (16,16)->(1,1) of the case table is 16 : 1: the
    restatement and Pillow are compared on it like on the rest, the library must refuse it, and (8,8)->(1,1) stands beside it as the
    one-pixel output the kernels compute."""
    return all(a <= MAX_RATIO * b and b <= MAX_RATIO * a for a, b in zip(in_size, out_size))


DEVICE_CASES = [case for case in CASES if in_range(*case)]
REFUSED_CASES = [case for case in CASES if not in_range(*case)]
PATTERNS = ("noise", "checker")


@functools.lru_cache(maxsize=None)
def pattern(name, h, w):
    """uniform-random uint8 noise; a 0/255 checkerboard, which drives both ends of clip8 through the negative lobes."""
    if name == "noise":
        img = np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2).copy()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(name, in_size, out_size, filter):
    """The restatement's result of a case, computed once and shared (read-only)."""
    out = resize_u8(pattern(name, *in_size), out_size[0], out_size[1], filter)
    out.setflags(write=False)
    return out


def axis_pairs():
    """Every (in, out) pair the coefficient test covers: those of the cases and 1..40 x 1..40 within the ratio limit."""
    pairs = {(a, b) for a in range(1, 41) for b in range(1, 41) if a <= MAX_RATIO * b and b <= MAX_RATIO * a}
    for (h_in, w_in), (h_out, w_out) in DEVICE_CASES:
        pairs.update({(h_in, h_out), (w_in, w_out)})
    return sorted(pairs)
