"""Pillow-exact resize of 8-bit RGB images by any ratio up to 8 either way on the GPU (engine extension, absent upstream) -
``srgd_resize_u8_images`` of ``libsrgd_resize.so`` (srgd_amd/csrc/resize.hip, the definition is fixed in include/srgd_resize.h; a
library of its own beside the seven others, built by the same srgd_amd/build.py).  The result is ``Image.resize((w_out, h_out),
BICUBIC | BILINEAR | LANCZOS)`` bit for bit: the tables come from the library's host function (Pillow's doubles), the two passes are
integer kernels.  ``--outscale S`` of the folder driver resamples every x4 output with it immediately before the file is encoded.
There is no CPU path and no torch arithmetic here: torch allocates the buffers, uploads the tables and packs the images of a list."""
from __future__ import annotations

import ctypes as C
import functools
import math
import os

import numpy as np
import torch

from . import _flat, _lib
from ._flat import ALIGN, round16

FILTERS = {"bicubic": 3, "bilinear": 2, "lanczos": 1}     # name -> the library's number (PIL.Image.Resampling's)
MAX_SIDE = 16384
MAX_RATIO = 8
MAX_TAPS = 49
SCALE = 4                                                 # the network's factor: --outscale 4 is the output as it is
OUTSCALE_MIN, OUTSCALE_MAX = 0.5, 32.0
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsrgd_resize.so")


class ResizeImage(C.Structure):
    """``srgd_resize_image`` of include/srgd_resize.h."""
    _fields_ = [("src_off", C.c_int64), ("dst_off", C.c_int64), ("tab_off", C.c_int64),
                ("h_in", C.c_int32), ("w_in", C.c_int32), ("h_out", C.c_int32), ("w_out", C.c_int32)]


# name -> (restype, argtypes); every symbol include/srgd_resize.h declares
PROTOTYPES = {
    "srgd_resize_last_error": (C.c_char_p, []),
    "srgd_resize_ksize": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "srgd_resize_coeffs": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "srgd_resize_u8_images": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ResizeImage), C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_int64, C.c_void_p]),
}
_handle = None


def lib() -> C.CDLL:
    """Load the resize library (once).  Raises if it has not been built - no CPU fallback."""
    global _handle
    if _handle is None:
        _handle = _lib.load(LIB_PATH, PROTOTYPES, "The resize runs on the MI355X only")
    return _handle


def _error():
    return _lib.error_of(lib(), "srgd_resize_last_error")


def check_filter(name):
    """``None`` -> "bicubic" (the operator that made the model's conditions); a name of ``FILTERS`` -> that name; anything else
    raises ``ValueError``."""
    if name is None:
        return "bicubic"
    if not isinstance(name, str) or name not in FILTERS:
        raise ValueError(f"resize: filter must be one of {', '.join(FILTERS)}, got {name!r}")
    return name


def check_outscale(s):
    """``None`` / 4 -> None (no resize: the network's x4 output as it is); a finite number in [0.5, 32] -> the float; anything else
    raises ``ValueError``."""
    if s is None:
        return None
    if isinstance(s, bool) or not isinstance(s, (int, float)) or not OUTSCALE_MIN <= s <= OUTSCALE_MAX:      # NaN fails both comparisons
        raise ValueError(f"outscale: S must be a number in [{OUTSCALE_MIN}, {OUTSCALE_MAX:g}] ({SCALE}: off), got {s!r}")
    return None if float(s) == SCALE else float(s)


def outscale_size(h_lr, w_lr, s):
    """Output size of an ``h_lr`` x ``w_lr`` input at output scale ``s``: ``max(1, floor(in * s + 0.5))`` per axis."""
    return tuple(max(1, int(math.floor(n * s + 0.5))) for n in (h_lr, w_lr))


def ksize(in_size, out_size, filter="bicubic"):
    """Taps of a row of the table ``in_size`` -> ``out_size`` (host only).  ``ValueError`` for what the library refuses."""
    k = lib().srgd_resize_ksize(int(in_size), int(out_size), FILTERS[check_filter(filter)])
    if k < 0:
        raise ValueError(str(_error()))
    return k


@functools.lru_cache(maxsize=64)
def _table(in_size, out_size, filter):
    k = ksize(in_size, out_size, filter)
    tab = np.zeros(out_size * (2 + k), np.int32)          # bounds[out][2], then coeffs[out][ksize]: the layout the kernels read
    if lib().srgd_resize_coeffs(in_size, out_size, FILTERS[filter], C.c_void_p(tab.ctypes.data),
                                C.c_void_p(tab[2 * out_size:].ctypes.data)) != 0:
        raise ValueError(str(_error()))
    tab.setflags(write=False)
    return tab


def coeffs(in_size, out_size, filter="bicubic"):
    """The table ``in_size`` -> ``out_size`` as the library computes it (host only, Pillow's doubles): ``(bounds [out,2] int32 =
    (first input, taps), coeffs [out,ksize] int32 in 22-bit fixed point, zero beyond the taps)``."""
    tab = _table(int(in_size), int(out_size), check_filter(filter))
    return tab[:2 * out_size].reshape(out_size, 2).copy(), tab[2 * out_size:].reshape(out_size, -1).copy()


def scratch_bytes(sizes):
    """Bytes of the scratch the C entry needs for ``[(h_in, w_in, h_out, w_out)]`` (include/srgd_resize.h: per image the horizontal
    pass's ``3 * h_in * w_out`` bytes, rounded up to a multiple of 16)."""
    return sum(round16(3 * h_in * w_out) for (h_in, _, _, w_out) in sizes)


def check_sizes(sizes):
    """``ValueError`` unless every ``(h_in, w_in, h_out, w_out)`` is a geometry the kernels take: every size in 1 .. 16384 and, per
    axis, a ratio of at most 8 either way."""
    for (h_in, w_in, h_out, w_out) in sizes:
        for a, b in ((h_in, h_out), (w_in, w_out)):
            if not (1 <= a <= MAX_SIDE and 1 <= b <= MAX_SIDE and a <= MAX_RATIO * b and b <= MAX_RATIO * a):
                raise ValueError(f"resize: {h_in}x{w_in} -> {h_out}x{w_out} is outside what the kernels take (sizes in 1 .. {MAX_SIDE}, "
                                 f"per axis a ratio of at most {MAX_RATIO} either way)")


def build_tables(sizes, filter="bicubic"):
    """The host side of the device table buffer for ``[(h_in, w_in, h_out, w_out)]``: ``(int32 array, [byte offset of image i's
    tables])`` - per image the table ``w_in -> w_out`` where the widths differ, directly followed by the table ``h_in -> h_out``
    where the heights differ; every image's offset is a multiple of 16.  Images of one geometry share their tables."""
    filter = check_filter(filter)
    check_sizes(sizes)
    parts, offsets, seen, total = [], [], {}, 0
    for size in sizes:
        if size not in seen:
            h_in, w_in, h_out, w_out = size
            seen[size] = total
            for a, b in ((w_in, w_out), (h_in, h_out)):
                if a != b:
                    parts.append(_table(a, b, filter))
                    total += 4 * parts[-1].size
            pad = round16(total) - total
            if pad:
                parts.append(np.zeros(pad // 4, np.int32))
                total += pad
        offsets.append(seen[size])
    return (np.concatenate(parts) if parts else np.zeros(0, np.int32)), offsets


def resize_flat(src, src_offsets, dst, dst_offsets, sizes, filter="bicubic"):
    """One batched call on flat uint8 device buffers: image i's ``[h_in,w_in,3]`` bytes start at ``src_offsets[i]`` of ``src``, its
    result ``[h_out,w_out,3]`` at ``dst_offsets[i]`` of ``dst`` (offsets are multiples of 16), ``sizes`` = ``[(h_in, w_in, h_out,
    w_out)]``.  The tables are computed on the host and uploaded; the scratch is allocated here.  Returns ``dst``.  No
    synchronisation."""
    filter = check_filter(filter)
    # check_flat's two halves, apart: the buffers are refused before the sizes are, the spans after, and the first message says
    # "the resize" where the others say "resize" - the order and the words the callers and the tests know
    _flat.check_buffers("resize", (src, dst), subject="the resize")
    sizes = [tuple(int(v) for v in size) for size in sizes]
    n = len(sizes)
    check_sizes(sizes)
    _flat.check_spans("resize", n, (src, src_offsets, [3 * s[0] * s[1] for s in sizes]), (dst, dst_offsets, [3 * s[2] * s[3] for s in sizes]))
    host_tables, tab_offsets = build_tables(sizes, filter)
    tables = torch.from_numpy(np.concatenate([host_tables, np.zeros(4, np.int32)])).to(src.device)       # never empty
    scratch = torch.empty(max(scratch_bytes(sizes), ALIGN), device=src.device, dtype=torch.uint8)
    images = (ResizeImage * n)(*[ResizeImage(so, do, to, *size) for so, do, to, size in zip(src_offsets, dst_offsets, tab_offsets, sizes)])
    with torch.cuda.device(src.device):
        rc = lib().srgd_resize_u8_images(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), images, n, FILTERS[filter],
                                         C.c_void_p(tables.data_ptr()), 4 * tables.numel(), C.c_void_p(scratch.data_ptr()),
                                         scratch.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _error()
    return dst


def resize_on_device(images, sizes, filter="bicubic"):
    """``images``: a list of uint8 ``[H_i,W_i,3]`` tensors (moved to the GPU if they are not there), ``sizes``: one ``(h_out, w_out)``
    per image -> a list of uint8 ``[h_out,w_out,3]`` device tensors, ``Image.resize((w_out, h_out), filter)`` of each bit for bit;
    every image in ONE batched call.  ``ValueError``: an unknown filter, shapes that are not ``[H,W,3]`` uint8, a size outside
    1 .. 16384 or a ratio above 8."""
    filter = check_filter(filter)
    if not isinstance(images, (list, tuple)) or not images or len(images) != len(sizes):
        raise ValueError("resize_on_device: a list of images and one (h_out, w_out) per image")
    for im in images:
        if not torch.is_tensor(im) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError("resize_on_device: images are uint8 [H,W,3] tensors")
    geo = [(int(im.shape[0]), int(im.shape[1]), int(h), int(w)) for im, (h, w) in zip(images, sizes)]
    check_sizes(geo)
    src, src_offsets = _flat.gather(images, _flat.device_of(images, "the resize"))
    dst_offsets, total = _flat.layout([3 * h * w for (_, _, h, w) in geo])
    dst = torch.empty(total, device=src.device, dtype=torch.uint8)
    resize_flat(src, src_offsets, dst, dst_offsets, geo, filter)
    return [dst[off:off + 3 * h * w].view(h, w, 3) for off, (_, _, h, w) in zip(dst_offsets, geo)]
