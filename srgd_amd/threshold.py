"""Dynamic thresholding inside the tiled DDPM sampling loop on the GPU (engine extension, absent upstream; Imagen's percentile
clipping) - ``srgd_threshold_step`` of ``libsrgd_threshold.so`` (srgd_amd/csrc/threshold.hip, the definition is fixed in
include/srgd_threshold.h; a library of its own beside the engine's and the eight other extension libraries, built by the same
srgd_amd/build.py).  After a step taken without the static clamp, every image's prediction of the clean image is clipped to [-s, s]
and divided by s - s >= 1 an exact quantile of its magnitudes inside the crop box, selected on the GPU by a radix select - and the
image canvas receives the change scaled by the posterior mean's weight of the prediction.
There is no CPU path and no torch arithmetic here: the caller owns the canvases, the output array and the scratch."""
from __future__ import annotations

import ctypes as C
import math
import os
import struct

import torch

from . import _lib

ALIGN = 256                             # the scratch is aligned to it
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsrgd_threshold.so")


class ThresholdImage(C.Structure):
    """``srgd_threshold_image`` of include/srgd_threshold.h."""
    _fields_ = [("canvas_off", C.c_int64), ("Hp", C.c_int32), ("Wp", C.c_int32), ("top", C.c_int32), ("left", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("box_t", C.c_int32), ("box_l", C.c_int32), ("box_h", C.c_int32),
                ("box_w", C.c_int32)]


# name -> (restype, argtypes); every symbol include/srgd_threshold.h declares
PROTOTYPES = {
    "srgd_threshold_last_error": (C.c_char_p, []),
    "srgd_threshold_position": (C.c_int, [C.c_int64, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_float)]),
    "srgd_threshold_scratch_bytes": (C.c_uint64, [C.c_int]),
    "srgd_threshold_chunk_elems": (C.c_int, []),
    "srgd_threshold_step": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ThresholdImage), C.c_int, C.c_float, C.c_float, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
}
_handle = None


def lib() -> C.CDLL:
    """Load the threshold library (once).  Raises if it has not been built - no CPU fallback."""
    global _handle
    if _handle is None:
        _handle = _lib.load(LIB_PATH, PROTOTYPES, "The dynamic threshold runs on the MI355X only")
    return _handle


def _error():
    return _lib.error_of(lib(), "srgd_threshold_last_error")


def fp32(v) -> float:
    """``v`` rounded to fp32, as a Python float."""
    return struct.unpack("f", struct.pack("f", v))[0]


def chunk_elems() -> int:
    """Keys of the statistics box one workgroup of the histogram kernels counts (host only)."""
    return int(lib().srgd_threshold_chunk_elems())


def position(n, q):
    """``(lo, hi, frac)`` of quantile ``q`` among ``n`` sorted values as the library computes it (host only)."""
    lo, hi, frac = C.c_int64(), C.c_int64(), C.c_float()
    if lib().srgd_threshold_position(int(n), float(q), C.byref(lo), C.byref(hi), C.byref(frac)) != 0:
        raise _error()
    return lo.value, hi.value, frac.value


def scratch_bytes(n_images) -> int:
    """Bytes of the scratch buffer the C entry needs for ``n_images`` images (host only)."""
    if isinstance(n_images, bool) or not isinstance(n_images, int) or n_images < 1:
        raise ValueError(f"dynamic_threshold: n_images must be an int >= 1, got {n_images!r}")
    return int(lib().srgd_threshold_scratch_bytes(n_images))


def check_percentile(p):
    """``tiled_sample``'s ``dynamic_threshold``: None / 0 -> None (no thresholding); a number whose fp32 rounding lies in (0, 1] ->
    that fp32 value as a float; anything else raises ``ValueError``."""
    if p is None:
        return None
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not math.isfinite(p):
        raise ValueError(f"dynamic_threshold: the percentile must be a number in [0, 1] (0: off), got {p!r}")
    if p == 0:
        return None
    q = fp32(p) if abs(p) < 3e38 else math.inf
    if not 0.0 < q <= 1.0:
        raise ValueError(f"dynamic_threshold: the percentile must be a number in [0, 1] (0: off), got {p!r}")
    return q


def records(images):
    """The host record array of a call: ``images`` = ``[(canvas_off, Hp, Wp, top, left, H, W, box_t, box_l, box_h, box_w)]`` - the
    statistics box (the crop box) and the update box (what the step wrote) -> ``ThresholdImage`` array.  ``ValueError`` for a box
    that leaves its frame."""
    if not images:
        raise ValueError("dynamic_threshold: no images")
    recs = (ThresholdImage * len(images))()
    for r, m in zip(recs, images):
        off, hp, wp, top, left, h, w, bt, bl, bh, bw = (int(v) for v in m)
        if off < 0 or h < 1 or w < 1 or bt < 0 or bl < 0 or bt + bh > hp or bl + bw > wp or top < bt or left < bl \
                or top + h > bt + bh or left + w > bl + bw or 3 * hp * wp >= 2 ** 31:
            raise ValueError(f"dynamic_threshold: bad canvas {hp}x{wp} / statistics box {h}x{w} at ({top}, {left}) / update box "
                             f"{bh}x{bw} at ({bt}, {bl}) / offset {off}")
        r.canvas_off, r.Hp, r.Wp, r.top, r.left, r.H, r.W, r.box_t, r.box_l, r.box_h, r.box_w = off, hp, wp, top, left, h, w, bt, bl, bh, bw
    return recs


def threshold_step_flat(img, x_start, recs, q, weight_img, s_out, scratch):
    """One batched call on flat fp32 device buffers, in place on ``img`` and ``x_start``: ``recs`` from ``records`` (image i's
    ``[3,Hp,Wp]`` canvas starts at ``canvas_off`` of ``img`` and ``x_start`` alike), ``s_out`` an fp32 device buffer of at least
    ``len(recs)`` elements that receives every image's s, ``scratch`` a uint8 device buffer of at least ``scratch_bytes(len(recs))``
    bytes.  No allocation, no synchronisation."""
    for v in (q, weight_img):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"dynamic_threshold: q and weight_img are numbers, got {v!r}")
    if not isinstance(recs, C.Array) or recs._type_ is not ThresholdImage or len(recs) < 1:
        raise ValueError("dynamic_threshold: recs is the record array records() returns")
    for t in (img, x_start, s_out):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("dynamic_threshold: contiguous fp32 buffers")
    if not torch.is_tensor(scratch) or scratch.dtype != torch.uint8 or not scratch.is_contiguous():
        raise ValueError("dynamic_threshold: the scratch is a contiguous uint8 buffer")
    if max(r.canvas_off + 3 * r.Hp * r.Wp for r in recs) > min(img.numel(), x_start.numel()) or s_out.numel() < len(recs) \
            or scratch_bytes(len(recs)) > scratch.numel():
        raise ValueError("dynamic_threshold: records do not fit the buffers")
    if len({img.device, x_start.device, s_out.device, scratch.device}) != 1:
        raise ValueError("dynamic_threshold: buffers on one device")
    if not img.is_cuda:
        raise _lib.SrgdHipError("the dynamic threshold runs on MI355X only (no CPU fallback)")
    with torch.cuda.device(img.device):
        rc = lib().srgd_threshold_step(C.c_void_p(img.data_ptr()), C.c_void_p(x_start.data_ptr()), recs, len(recs), float(q),
                                       float(weight_img), C.c_void_p(s_out.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _error()
