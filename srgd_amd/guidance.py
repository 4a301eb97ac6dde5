"""LR-consistency guidance inside the tiled DDPM sampling loop on the GPU (engine extension, absent upstream) -
``srgd_guidance_step`` of ``libsrgd_guidance.so`` (srgd_amd/csrc/guidance.hip, the definition is fixed in include/srgd_guidance.h; a
library of its own beside the engine's, the metrics', the ensemble's, the consistency's and the back-projection's, built by the same
srgd_amd/build.py).  After a step, the model's prediction of the clean image is reduced by 4 and enlarged by 4 again with the
coefficients of Pillow's bicubic in fp32, and the difference between the condition and that image is added to the prediction and,
scaled by the posterior mean's weight of the prediction, to the image canvas - inside every image's crop box only.
There is no CPU path and no torch arithmetic here: the caller owns the canvases and the scratch."""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from . import _lib

MIN_SIDE = 5                            # LR pixels: below it the clipped windows overlap and the coefficient rows depend on the size
SCALE = 4
ALIGN = 256                             # the scratch and every image's part of it are multiples of it
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsrgd_guidance.so")


class GuidanceImage(C.Structure):
    """``srgd_guidance_image`` of include/srgd_guidance.h."""
    _fields_ = [("canvas_off", C.c_int64), ("cond_off", C.c_int64), ("Hp", C.c_int32), ("Wp", C.c_int32), ("top", C.c_int32),
                ("left", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]


# name -> (restype, argtypes); every symbol include/srgd_guidance.h declares
PROTOTYPES = {
    "srgd_guidance_last_error": (C.c_char_p, []),
    "srgd_guidance_coeffs": (C.c_int, [C.c_void_p, C.c_void_p]),
    "srgd_guidance_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GuidanceImage), C.c_int, C.c_float, C.c_float,
                                     C.c_void_p, C.c_void_p]),
}
_handle = None


def lib() -> C.CDLL:
    """Load the guidance library (once).  Raises if it has not been built - no CPU fallback."""
    global _handle
    if _handle is None:
        _handle = _lib.load(LIB_PATH, PROTOTYPES, "The guidance runs on the MI355X only")
    return _handle


def coeffs():
    """The coefficient vectors as the kernels use them (host only): ``(down [5][16], up [16][4])`` lists of floats, each vector on
    the frame of its output (include/srgd_guidance.h)."""
    down, up = ((C.c_float * 16) * 5)(), ((C.c_float * 4) * 16)()
    if lib().srgd_guidance_coeffs(C.cast(down, C.c_void_p), C.cast(up, C.c_void_p)) != 0:
        raise _lib.error_of(lib(), "srgd_guidance_last_error")
    return [list(row) for row in down], [list(row) for row in up]


def check_weight(weight):
    """``tiled_sample``'s ``consistency_guidance``: None / 0 -> None (no guidance); a number in (0, 1] -> the float; anything else
    raises ``ValueError``."""
    if weight is None:
        return None
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not math.isfinite(weight) or not 0.0 <= weight <= 1.0:
        raise ValueError(f"consistency_guidance: the weight must be a number in [0, 1] (0: off), got {weight!r}")
    return float(weight) or None


def check_start_steps(start):
    """``consistency_guidance_start_steps``: an int >= 0."""
    if isinstance(start, bool) or not isinstance(start, int) or start < 0:
        raise ValueError(f"consistency_guidance_start_steps: an int >= 0, got {start!r}")
    return start


def check_hr_sizes(sizes):
    """``ValueError`` unless every ``(H, W)`` is the x4 output of an LR image the kernels take: multiples of 4, both >= 20.
    -> the LR sizes."""
    low = []
    for (hh, ww) in sizes:
        if hh % SCALE or ww % SCALE or hh < SCALE * MIN_SIDE or ww < SCALE * MIN_SIDE:
            raise ValueError(f"consistency_guidance: bad image size {hh}x{ww} (height and width are multiples of {SCALE} and at least "
                             f"{SCALE * MIN_SIDE})")
        low.append((hh // SCALE, ww // SCALE))
    return low


def _round(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def scratch_bytes(sizes):
    """Bytes of the scratch buffer the C entry needs for LR sizes ``[(h, w)]`` (include/srgd_guidance.h: per image D, [3][h][w] fp32
    = 12hw bytes, rounded up to a multiple of 256)."""
    for (h, w) in sizes:
        if h < MIN_SIDE or w < MIN_SIDE:
            raise ValueError(f"consistency_guidance: bad image size {h}x{w} (both sides must be >= {MIN_SIDE})")
    return sum(_round(12 * h * w) for (h, w) in sizes)


def records(images):
    """The host record array of a run: ``images`` = ``[(canvas_off, cond_off, Hp, Wp, top, left, H, W)]`` with the HR size of the
    crop box -> ``(GuidanceImage array, LR sizes)``.  ``ValueError`` for a size the kernels do not take or a crop box that leaves
    its canvas."""
    if not images:
        raise ValueError("consistency_guidance: no images")
    low = check_hr_sizes([(int(m[6]), int(m[7])) for m in images])
    recs = (GuidanceImage * len(images))()
    for r, m, (h, w) in zip(recs, images, low):
        canvas_off, cond_off, hp, wp, top, left = (int(v) for v in m[:6])
        if canvas_off < 0 or cond_off < 0 or top < 0 or left < 0 or top + SCALE * h > hp or left + SCALE * w > wp \
                or 3 * hp * wp >= 2 ** 31:
            raise ValueError(f"consistency_guidance: bad canvas {hp}x{wp} / crop box at ({top}, {left}) / offsets")
        r.canvas_off, r.cond_off, r.Hp, r.Wp, r.top, r.left, r.h, r.w = canvas_off, cond_off, hp, wp, top, left, h, w
    return recs, low


def guide_step_flat(img, x_start, cond01, recs, weight_x0, weight_img, scratch):
    """One batched call on flat fp32 device buffers, in place on ``img`` and ``x_start``: ``recs`` from ``records`` (image i's
    ``[3,Hp,Wp]`` canvas starts at ``canvas_off`` of ``img`` and ``x_start`` alike, its ``[3,H,W]`` condition at ``cond_off`` of
    ``cond01``), ``scratch`` a uint8 device buffer of at least ``scratch_bytes(LR sizes)`` bytes.  No allocation, no
    synchronisation."""
    for w_ in (weight_x0, weight_img):
        if isinstance(w_, bool) or not isinstance(w_, (int, float)) or not math.isfinite(w_):
            raise ValueError(f"consistency_guidance: the weights must be finite numbers, got {w_!r}")
    if not isinstance(recs, C.Array) or recs._type_ is not GuidanceImage or len(recs) < 1:
        raise ValueError("consistency_guidance: recs is the record array records() returns")
    for t in (img, x_start, cond01):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("consistency_guidance: contiguous fp32 buffers")
    if not torch.is_tensor(scratch) or scratch.dtype != torch.uint8 or not scratch.is_contiguous():
        raise ValueError("consistency_guidance: the scratch is a contiguous uint8 buffer")
    if max(r.canvas_off + 3 * r.Hp * r.Wp for r in recs) > min(img.numel(), x_start.numel()) \
            or max(r.cond_off + 48 * r.h * r.w for r in recs) > cond01.numel() \
            or scratch_bytes([(r.h, r.w) for r in recs]) > scratch.numel():
        raise ValueError("consistency_guidance: records do not fit the buffers")
    if len({img.device, x_start.device, cond01.device, scratch.device}) != 1:
        raise ValueError("consistency_guidance: buffers on one device")
    if not img.is_cuda:
        raise _lib.SrgdHipError("consistency guidance runs on MI355X only (no CPU fallback)")
    with torch.cuda.device(img.device):
        rc = lib().srgd_guidance_step(C.c_void_p(img.data_ptr()), C.c_void_p(x_start.data_ptr()), C.c_void_p(cond01.data_ptr()), recs,
                                      len(recs), float(weight_x0), float(weight_img), C.c_void_p(scratch.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _lib.error_of(lib(), "srgd_guidance_last_error")
