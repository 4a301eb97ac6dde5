"""Numpy restatements of what srgd_amd.alpha computes (include/srgd_alpha.h) and the case tables the CPU and the GPU tests share.

The plane resize is ``tests.resize_cases.table`` and ``_pass`` (Pillow's ``Resample.c`` in integers) applied to a ``[h,w]`` plane:
horizontal pass first, rounded to 8 bits, then the vertical pass; a pass whose in == out is skipped.  tests/test_alpha_cpu.py pins it
against Pillow's ``L`` resize and against band A of Pillow's RGBA resize on every case, filter and pattern below; the GPU tests
compare the kernels with it and never import Pillow's resize.  The pack is ``np.dstack``; the bleed is the Jacobi iteration of the
header in int64; ``attach`` composes them as ``--alpha keep`` does."""
from __future__ import annotations

import functools

import numpy as np

from tests import resize_cases as RC

H_TILE = (64, 16)                                            # horizontal plane kernel: output pixels x rows of a tile
V_TILE = (256, 16)                                           # vertical plane kernel: bytes x output rows of a tile
PACK_BLOCK = 4 * 256                                         # pixels of a workgroup of the pack and of the bleed's last kernel
MAX_BLEED = 64


def resize_plane(plane, out_h, out_w, filter):
    """uint8 [h,w] -> uint8 [out_h,out_w]: ``Image.fromarray(plane, "L").resize((out_w, out_h), FILTER)`` bit for bit."""
    h, w = plane.shape
    tmp = RC._pass(plane, *RC.table(w, out_w, filter), axis=1) if out_w != w else plane           # horizontal first
    return RC._pass(tmp, *RC.table(h, out_h, filter), axis=0) if out_h != h else tmp.copy()


def pack(rgb, alpha):
    """uint8 [h,w,3] + uint8 [h,w] -> uint8 [h,w,4]."""
    return np.dstack([rgb, alpha]).astype(np.uint8)


def bleed(rgba, passes):
    """uint8 [h,w,4] -> uint8 [h,w,3] after ``passes`` Jacobi passes: an unknown pixel with c >= 1 known 8-neighbours inside the
    image becomes ``(2 s + c) // (2 c)`` per channel (s their sum) and known; known = alpha > 0 at the start."""
    rgb = rgba[:, :, :3].astype(np.int64)
    known = rgba[:, :, 3] > 0
    h, w = known.shape
    for _ in range(passes):
        val = np.zeros((h + 2, w + 2, 3), np.int64)
        cnt = np.zeros((h + 2, w + 2), np.int64)
        val[1:-1, 1:-1] = rgb * known[:, :, None]
        cnt[1:-1, 1:-1] = known
        s = np.zeros((h, w, 3), np.int64)
        c = np.zeros((h, w), np.int64)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if (dy, dx) != (1, 1):
                    s += val[dy:dy + h, dx:dx + w]
                    c += cnt[dy:dy + h, dx:dx + w]
        fill = ~known & (c > 0)
        mean = (2 * s + c[:, :, None]) // np.maximum(2 * c, 1)[:, :, None]
        rgb = np.where(fill[:, :, None], mean, rgb)
        known = known | fill
    return rgb.astype(np.uint8)


def attach(rgb, alpha_lr, scale=4, filter="bicubic"):
    """uint8 [H,W,3] + the uint8 [h,w] plane of its input -> uint8 [H,W,4]: the plane x``scale`` with bicubic, then - where (H, W) is
    not x``scale`` of (h, w) - resized to (H, W) with ``filter``, then interleaved."""
    h, w = alpha_lr.shape
    a = resize_plane(alpha_lr, scale * h, scale * w, "bicubic")
    if a.shape != rgb.shape[:2]:
        a = resize_plane(a, rgb.shape[0], rgb.shape[1], filter)
    return pack(rgb, a)


# ((h_in, w_in), (h_out, w_out)): every geometry of the RGB resize that the library takes, and
PLANE_CASES = list(RC.DEVICE_CASES) + [
    # the smallest plane at x4; x4 of widths with w % 4 in {1, 2, 3, 0}; the two-stage path of a 10x13 input (its second stages,
    # (40,52)->(20,26) and ->(30,39), are among the cases above)
    ((1, 1), (4, 4)), ((3, 5), (12, 20)), ((2, 6), (8, 24)), ((3, 7), (12, 28)), ((2, 8), (8, 32)), ((10, 13), (40, 52)),
    # output widths with w % 4 in {1, 2, 3} from an input width with w % 4 == 0, and the other way round
    ((6, 12), (5, 9)), ((6, 12), (7, 10)), ((6, 12), (4, 11)), ((5, 9), (6, 12)),
    # the horizontal kernel's tile of 64 output pixels x 16 rows: tile - 1, tile, tile + 1
    ((17, 80), (15, 63)), ((15, 90), (16, 64)), ((16, 100), (17, 65)),
    # the vertical kernel's tile of 256 bytes x 16 output rows: 255, 256 and 257 bytes; 260 is a dword row that ends in its second tile
    ((9, 300), (12, 255)), ((9, 128), (12, 256)), ((9, 300), (7, 257)), ((20, 130), (17, 260)),
    # one pass skipped each way past a tile, and the copy past a tile of both kernels
    ((18, 70), (18, 66)), ((18, 264), (33, 264)), ((18, 264), (18, 264)), ((17, 65), (17, 65)),
]
SMALLEST = ((1, 1), (4, 4))
TWO_STAGE = [((10, 13), (20, 26)), ((10, 13), (30, 39))]      # LR plane, final size: via (40, 52)
PATTERNS = ("noise", "checker")
PACK_SIZES = [(1, 1), (1, 2), (1, 3), (2, 2), (5, 5), (3, 6), (7, 5), (16, 64), (31, 33), (33, 65)]      # h * w % 4: 1 2 3 0 1 2 3 0 3 1
BLEED_SIZES = [(1, 1), (1, 9), (7, 5), (33, 65)]
BLEED_PATTERNS = ("random70", "corner", "transparent", "opaque", "one_254")
BLEED_PASSES = (0, 1, 2, 5, 64)


@functools.lru_cache(maxsize=None)
def plane(name, h, w):
    """uniform-random uint8 noise; a 0/255 checkerboard, which drives both ends of clip8 through the negative lobes."""
    if name == "noise":
        p = np.random.default_rng(7000 * h + w).integers(0, 256, (h, w), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        p = (((yy + xx) & 1) * 255).astype(np.uint8)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def expected_plane(name, in_size, out_size, filter):
    """The restatement's result of a plane case, computed once and shared (read-only)."""
    out = resize_plane(plane(name, *in_size), out_size[0], out_size[1], filter)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def colour(h, w):
    img = np.random.default_rng(9000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def bleed_image(name, h, w):
    """uint8 [h,w,4]: random colour under an alpha plane of the named pattern - about 70 % zeros at random; one opaque pixel in the
    last corner; all transparent; all opaque; zeros, ones and 254s at random (1 is known, which pins ``> 0``)."""
    rng = np.random.default_rng(11000 * h + w)
    if name == "random70":
        a = np.where(rng.random((h, w)) < 0.7, 0, rng.integers(1, 256, (h, w)))
    elif name == "corner":
        a = np.zeros((h, w), np.int64)
        a[h - 1, w - 1] = 255
    elif name == "transparent":
        a = np.zeros((h, w), np.int64)
    elif name == "opaque":
        a = np.full((h, w), 255, np.int64)
    else:
        a = rng.choice(np.array([0, 0, 0, 1, 254]), (h, w))
    img = np.dstack([colour(h, w), a.astype(np.uint8)])
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected_bleed(name, h, w, passes):
    out = bleed(bleed_image(name, h, w), passes)
    out.setflags(write=False)
    return out


def chebyshev_to_known(alpha):
    """[h,w] int: every pixel's Chebyshev distance to the nearest pixel with alpha > 0 (a large number where there is none)."""
    h, w = alpha.shape
    ys, xs = np.nonzero(alpha > 0)
    if len(ys) == 0:
        return np.full((h, w), 1 << 30)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.maximum(np.abs(yy[:, :, None] - ys), np.abs(xx[:, :, None] - xs)).min(axis=2)
