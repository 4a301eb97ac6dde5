"""LR consistency (LR-PSNR) of x4 outputs against their own low-resolution inputs on the GPU (engine extension, absent upstream) -
``srgd_image_consistency_images`` of ``libsrgd_consistency.so`` (srgd_amd/csrc/consistency.hip, the definition is fixed in
include/srgd_consistency.h; a library of its own beside the engine's, the metrics' and the ensemble's, built by the same
srgd_amd/build.py).  The output as saved is reduced by 4 with Pillow's ``Image.resize(BICUBIC)`` - the operator that made the condition
- and compared with the input: inputs and outputs are uint8, so the kernel's results are exact integers.
There is no CPU path and no torch arithmetic here: torch allocates the buffers and copies the images into the padded layout, one copy
of ``4 * n`` integers per call brings the sums to the host, and the host derives the three numbers in float64."""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from . import _lib

VEC = 16                                # offsets of the images in the flat buffers are multiples of it
TILE_W, TILE_H = 32, 15                 # LR pixels of a tile = of one 32-byte record of the scratch (consistency.hip: CS_TW, CS_TH)
MIN_SIDE = 5                            # below it the clipped windows overlap and the coefficient rows depend on the size
SCALE = 4
KEYS = ("lr_psnr", "lr_mse", "lr_max_abs")
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsrgd_consistency.so")
# name -> (restype, argtypes); every symbol include/srgd_consistency.h declares
PROTOTYPES = {
    "srgd_image_consistency_last_error": (C.c_char_p, []),
    "srgd_image_consistency_coeffs": (C.c_int, [C.c_void_p]),
    "srgd_image_consistency": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "srgd_image_consistency_images": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                                C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p]),
}
_handle = None


def lib() -> C.CDLL:
    """Load the consistency library (once).  Raises if it has not been built - no CPU fallback."""
    global _handle
    if _handle is None:
        _handle = _lib.load(LIB_PATH, PROTOTYPES, "The consistency runs on the MI355X only")
    return _handle


def padded(n):
    """``n`` rounded up to a multiple of 16: the distance between two images of a packed flat buffer."""
    return (n + VEC - 1) // VEC * VEC


def coeffs():
    """The five coefficient vectors of the x4 reduction as the library computes them (host only): ``[5][16]`` ints, rows 0, 1,
    interior, n-2, n-1, each from its first tap on, zero beyond its last."""
    out = ((C.c_int32 * 16) * 5)()
    if lib().srgd_image_consistency_coeffs(C.cast(out, C.c_void_p)) != 0:
        raise _lib.error_of(lib(), "srgd_image_consistency_last_error")
    return [list(row) for row in out]


def scratch_bytes(sizes):
    """Bytes of the scratch buffer the C entry needs for LR sizes ``[(h, w)]`` (include/srgd_consistency.h: one 32-byte record per
    tile of 32 x 15 LR pixels)."""
    for (h, w) in sizes:
        if h < MIN_SIDE or w < MIN_SIDE:
            raise ValueError(f"consistency: bad image size {h}x{w} (both sides must be >= {MIN_SIDE})")
    return sum(32 * ((h + TILE_H - 1) // TILE_H) * ((w + TILE_W - 1) // TILE_W) for (h, w) in sizes)


def consistency_flat_device(hr_u8, hr_offsets, lr_u8, lr_offsets, sizes, down_u8=None, down_offsets=None):
    """One batched call on flat device buffers; returns the device tensor ``[n, 4]`` int64 of (sse_r, sse_g, sse_b, max_abs) without
    synchronising.  ``sizes``: the LR sizes ``(h_i, w_i)``; ``hr_u8``: uint8, output i is ``[4h_i,4w_i,3]`` from byte
    ``hr_offsets[i]``; ``lr_u8``: uint8, input i is ``[h_i,w_i,3]`` from byte ``lr_offsets[i]``; ``down_u8`` (optional): uint8, the
    reduced output ``[h_i,w_i,3]`` is written from byte ``down_offsets[i]``.  All offsets are multiples of 16."""
    if not (hr_u8.is_cuda and lr_u8.is_cuda and (down_u8 is None or down_u8.is_cuda)):
        raise _lib.SrgdHipError("the consistency runs on MI355X only (no CPU fallback)")
    bufs = [hr_u8, lr_u8] + ([down_u8] if down_u8 is not None else [])
    if any(b.dtype != torch.uint8 or not b.is_contiguous() or b.device != hr_u8.device for b in bufs):
        raise ValueError("consistency: contiguous uint8 output, input (and reduced-output) buffers on one device")
    if (down_u8 is None) != (down_offsets is None):
        raise ValueError("consistency: down_u8 and its offsets are given together")
    n = len(sizes)
    if n < 1 or len(hr_offsets) != n or len(lr_offsets) != n or (down_offsets is not None and len(down_offsets) != n):
        raise ValueError("consistency: at least one image, and one output offset and one input offset per image")
    sizes = [(int(h), int(w)) for (h, w) in sizes]
    n_scratch = scratch_bytes(sizes)
    elems = [3 * h * w for (h, w) in sizes]
    if min(hr_offsets) < 0 or min(lr_offsets) < 0 or max(o + SCALE * SCALE * e for o, e in zip(hr_offsets, elems)) > hr_u8.numel() \
            or max(o + e for o, e in zip(lr_offsets, elems)) > lr_u8.numel() \
            or (down_u8 is not None and (min(down_offsets) < 0 or max(o + e for o, e in zip(down_offsets, elems)) > down_u8.numel())):
        raise ValueError("consistency: offsets / sizes do not fit the buffers")
    stats = torch.empty(n, 4, device=hr_u8.device, dtype=torch.int64)
    scratch = torch.empty(n_scratch // 8, device=hr_u8.device, dtype=torch.int64)
    h_offs = (C.c_int64 * n)(*hr_offsets)
    l_offs = (C.c_int64 * n)(*lr_offsets)
    d_offs = (C.c_int64 * n)(*down_offsets) if down_u8 is not None else None
    hw = (C.c_int32 * (2 * n))(*[v for size in sizes for v in size])
    with torch.cuda.device(hr_u8.device):
        rc = lib().srgd_image_consistency_images(C.c_void_p(hr_u8.data_ptr()), h_offs, C.c_void_p(lr_u8.data_ptr()), l_offs, hw, n,
                                                 C.c_void_p(down_u8.data_ptr()) if down_u8 is not None else None, d_offs,
                                                 C.c_void_p(stats.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _lib.error_of(lib(), "srgd_image_consistency_last_error")
    return stats


def record(sse_r, sse_g, sse_b, max_abs, h, w):
    """The three numbers of one image from its four integers, in float64 (include/srgd_consistency.h)."""
    mse = (int(sse_r) + int(sse_g) + int(sse_b)) / (3 * h * w)
    return {"lr_psnr": math.inf if mse == 0 else 10.0 * math.log10(255.0 * 255.0 / mse), "lr_mse": mse, "lr_max_abs": float(max_abs)}


def records(stats, sizes):
    """The device ``[n, 4]`` result of ``consistency_flat_device`` as a list of ``{"lr_psnr", "lr_mse", "lr_max_abs"}`` dicts of
    Python floats: the one device-to-host copy of a group."""
    return [record(*row, h, w) for row, (h, w) in zip(stats.cpu().tolist(), sizes)]


def consistency_flat(hr_u8, hr_offsets, lr_u8, lr_offsets, sizes, down_u8=None, down_offsets=None):
    """``consistency_flat_device`` brought to the host: a list of ``{"lr_psnr", "lr_mse", "lr_max_abs"}`` dicts of Python floats."""
    return records(consistency_flat_device(hr_u8, hr_offsets, lr_u8, lr_offsets, sizes, down_u8, down_offsets), sizes)


def consistency_on_device(outputs, inputs, return_down=False):
    """LR consistency of every output against its own input: ``outputs`` is a uint8 ``[4h,4w,3]`` tensor on the GPU with ``inputs`` a
    uint8 ``[h,w,3]`` tensor, or both are lists (tuples) of such tensors, sizes free - every image of a list in ONE batched call.
    Returns, per image, ``{"lr_psnr", "lr_mse", "lr_max_abs"}`` - one dict for a tensor, a list of them for a list - or, where
    ``return_down`` is set, the pair ``(dict, D)`` with ``D`` the uint8 ``[h,w,3]`` reduced output.
    ``ValueError``: shapes, dtypes or sizes that do not fit, ``h`` or ``w`` below 5."""
    single = torch.is_tensor(outputs)
    if single != torch.is_tensor(inputs):
        raise ValueError("consistency_on_device: a tensor takes a tensor, a list takes a list")
    outs = [outputs] if single else (list(outputs) if isinstance(outputs, (list, tuple)) else None)
    ins = [inputs] if single else (list(inputs) if isinstance(inputs, (list, tuple)) else None)
    if not outs or not ins or len(outs) != len(ins):
        raise ValueError("consistency_on_device: uint8 [4h,4w,3] outputs and as many uint8 [h,w,3] inputs (tensors or non-empty lists)")
    for o, l in zip(outs, ins):
        if not torch.is_tensor(o) or not torch.is_tensor(l) or o.dtype != torch.uint8 or l.dtype != torch.uint8 \
                or o.dim() != 3 or l.dim() != 3 or o.shape[2] != 3 or l.shape[2] != 3:
            raise ValueError("consistency_on_device: every output is a uint8 [4h,4w,3] tensor, every input a uint8 [h,w,3] tensor")
        h, w = int(l.shape[0]), int(l.shape[1])
        if (int(o.shape[0]), int(o.shape[1])) != (SCALE * h, SCALE * w):
            raise ValueError(f"consistency_on_device: the output of a {h}x{w} input is {SCALE * h}x{SCALE * w}, got "
                             f"{int(o.shape[0])}x{int(o.shape[1])}")
        if h < MIN_SIDE or w < MIN_SIDE:
            raise ValueError(f"consistency_on_device: a {h}x{w} input is too small (both sides must be >= {MIN_SIDE})")
    dev = outs[0].device
    if not all(t.is_cuda and t.device == dev for t in outs + ins):
        raise _lib.SrgdHipError("the consistency runs on MI355X only (no CPU fallback): outputs and inputs are tensors of one GPU")
    sizes = [(int(l.shape[0]), int(l.shape[1])) for l in ins]
    elems = [3 * h * w for (h, w) in sizes]
    h_offs, l_offs, h_total, l_total = [], [], 0, 0
    for e in elems:
        h_offs.append(h_total)
        l_offs.append(l_total)
        h_total += padded(SCALE * SCALE * e)
        l_total += padded(e)
    hr = torch.empty(h_total, device=dev, dtype=torch.uint8)
    lr = torch.empty(l_total, device=dev, dtype=torch.uint8)
    for o, l, ho, lo, e in zip(outs, ins, h_offs, l_offs, elems):        # the padding stays as it is and is never read
        hr[ho:ho + SCALE * SCALE * e].copy_(o.reshape(-1))
        lr[lo:lo + e].copy_(l.reshape(-1))
    down = torch.empty(l_total, device=dev, dtype=torch.uint8) if return_down else None
    recs = consistency_flat(hr, h_offs, lr, l_offs, sizes, down, l_offs if return_down else None)
    if return_down:
        recs = [(rec, down[lo:lo + e].view(h, w, 3)) for rec, lo, e, (h, w) in zip(recs, l_offs, elems, sizes)]
    return recs[0] if single else recs
