"""Iterative back-projection of x4 outputs onto their own low-resolution inputs on the GPU (engine extension, absent upstream) -
``srgd_image_backproject_images`` of ``libsrgd_backproject.so`` (srgd_amd/csrc/backproject.hip, the definition is fixed in
include/srgd_backproject.h; a library of its own beside the engine's, the metrics', the ensemble's and the consistency's, built by the
same srgd_amd/build.py).  The output as saved is reduced by 4 and enlarged by 4 again with Pillow's ``Image.resize(BICUBIC)``, the
difference between the condition and that image is added, N times: everything between the two quantisations is uint8, so the
kernels' results are exact integers.
There is no CPU path and no torch arithmetic here: torch allocates the result and the scratch, and packs the images of a list."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib

MIN_SIDE = 5                            # LR pixels: below it the clipped windows overlap and the coefficient rows depend on the size
SCALE = 4
MAX_ITERATIONS = 64
ALIGN = 256                             # the scratch and its three parts per image are multiples of it
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsrgd_backproject.so")
# name -> (restype, argtypes); every symbol include/srgd_backproject.h declares
PROTOTYPES = {
    "srgd_image_backproject_last_error": (C.c_char_p, []),
    "srgd_image_backproject_coeffs": (C.c_int, [C.c_void_p]),
    "srgd_image_backproject": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "srgd_image_backproject_images": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
}
_handle = None


def lib() -> C.CDLL:
    """Load the back-projection library (once).  Raises if it has not been built - no CPU fallback."""
    global _handle
    if _handle is None:
        _handle = _lib.load(LIB_PATH, PROTOTYPES, "The back-projection runs on the MI355X only")
    return _handle


def coeffs():
    """The sixteen coefficient vectors of the x4 enlargement as the library computes them (host only): ``[16][4]`` ints - output
    indices 0 .. 5, the four phases of the interior, output indices 4n-6 .. 4n-1 - each from its first tap on, zero beyond its last."""
    out = ((C.c_int32 * 4) * 16)()
    if lib().srgd_image_backproject_coeffs(C.cast(out, C.c_void_p)) != 0:
        raise _lib.error_of(lib(), "srgd_image_backproject_last_error")
    return [list(row) for row in out]


def check_iterations(n):
    """``None`` / 0 -> None (no back-projection); 1 .. 64 -> the int; anything else raises ``ValueError``."""
    if n is None:
        return None
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= MAX_ITERATIONS:
        raise ValueError(f"back_project: iterations must be an int in 0 .. {MAX_ITERATIONS} (0: off), got {n!r}")
    return n or None


def check_hr_sizes(sizes):
    """``ValueError`` unless every ``(H, W)`` is the x4 output of an LR image the kernels take: multiples of 4, both >= 20, and
    ``3 * H * W < 2^31 - 256`` elements (include/srgd_backproject.h).  -> the LR sizes."""
    low = []
    for (hh, ww) in sizes:
        if hh % SCALE or ww % SCALE or hh < SCALE * MIN_SIDE or ww < SCALE * MIN_SIDE or 3 * hh * ww >= 2 ** 31 - 256:
            raise ValueError(f"back_project: bad image size {hh}x{ww} (height and width are multiples of {SCALE}, at least "
                             f"{SCALE * MIN_SIDE}, and 3*H*W < 2^31 - 256)")
        low.append((hh // SCALE, ww // SCALE))
    return low


def _round(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def scratch_bytes(sizes):
    """Bytes of the scratch buffer the C entry needs for LR sizes ``[(h, w)]`` (include/srgd_backproject.h: per image O and C of
    48hw bytes and D of 3hw bytes, each rounded up to a multiple of 256)."""
    for (h, w) in sizes:
        if h < MIN_SIDE or w < MIN_SIDE:
            raise ValueError(f"back_project: bad image size {h}x{w} (both sides must be >= {MIN_SIDE})")
    return sum(2 * _round(48 * h * w) + _round(3 * h * w) for (h, w) in sizes)


def back_project_flat(out, cond, offsets, sizes, iterations, dst=None):
    """One batched call on flat fp32 device buffers: image i's ``[3,H_i,W_i]`` planes start at ``offsets[i]`` of ``out``, ``cond``
    and ``dst`` alike, ``sizes`` are the HR sizes ``(H_i, W_i)`` (``dst=None``: in place, the result replaces ``out``).  Returns
    ``dst``.  No synchronisation."""
    iterations = check_iterations(iterations)
    if iterations is None:
        raise ValueError("back_project_flat needs iterations in 1 .. 64")
    if not (out.is_cuda and cond.is_cuda):
        raise _lib.SrgdHipError("back-projection runs on MI355X only (no CPU fallback)")
    dst = out if dst is None else dst
    for t in (out, cond, dst):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != out.device:
            raise ValueError("back_project: contiguous fp32 buffers on one device")
    n = len(sizes)
    low = check_hr_sizes([(int(hh), int(ww)) for (hh, ww) in sizes])
    if len(offsets) != n or n < 1 or min(offsets) < 0 \
            or max(off + 48 * h * w for off, (h, w) in zip(offsets, low)) > min(out.numel(), cond.numel(), dst.numel()):
        raise ValueError("back_project: offsets / sizes do not fit the buffers")
    scratch = torch.empty(scratch_bytes(low), device=out.device, dtype=torch.uint8)
    offs = (C.c_int64 * n)(*offsets)
    hw = (C.c_int32 * (2 * n))(*[v for size in low for v in size])
    with torch.cuda.device(out.device):
        rc = lib().srgd_image_backproject_images(C.c_void_p(out.data_ptr()), C.c_void_p(cond.data_ptr()), offs, hw, n, iterations,
                                                 C.c_void_p(dst.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _lib.error_of(lib(), "srgd_image_backproject_last_error")
    return dst


def back_project_on_device(out, cond, iterations):
    """``out`` pulled back onto ``cond`` by ``iterations`` (1 .. 64) back-projection steps, both fp32 in [0,1] on the GPU:

    * tensors ``[3,H,W]``, ``[1,3,H,W]`` or ``[B,3,H,W]`` of one shape -> a new tensor of that shape;
    * lists (tuples) of ``[1,3,H_i,W_i]`` tensors, sizes free -> a list of new ``[1,3,H_i,W_i]`` tensors;

    every image in ONE batched call (the images of a list are packed into flat buffers first).  ``out`` is left as it is.
    ``ValueError``: iterations outside 1 .. 64, shapes that do not match, H or W no multiple of 4 or below 20."""
    if check_iterations(iterations) is None:
        raise ValueError(f"back_project_on_device: iterations must be in 1 .. {MAX_ITERATIONS}, got {iterations!r}")
    if isinstance(out, (list, tuple)) != isinstance(cond, (list, tuple)):
        raise ValueError("back_project_on_device: out and cond are both tensors or both lists")
    if isinstance(out, (list, tuple)):
        if len(out) != len(cond) or not out:
            raise ValueError("back_project_on_device: one condition per output")
        for o, c in zip(out, cond):
            if not (torch.is_tensor(o) and torch.is_tensor(c)) or o.dim() != 4 or o.shape[0] != 1 or o.shape[1] != 3 \
                    or o.shape != c.shape:
                raise ValueError("back_project_on_device: lists hold matching [1,3,H,W] tensors")
        dev = out[0].device
        sizes = [(int(o.shape[2]), int(o.shape[3])) for o in out]
        check_hr_sizes(sizes)
        if dev.type != "cuda":
            raise _lib.SrgdHipError("back-projection runs on MI355X only (no CPU fallback)")
        offsets, total = [], 0
        for (h, w) in sizes:
            offsets.append(total)
            total += 3 * h * w
        flat_out = torch.cat([o.to(dev, torch.float32).reshape(-1) for o in out])
        flat_cond = torch.cat([c.to(dev, torch.float32).reshape(-1) for c in cond])
        back_project_flat(flat_out, flat_cond, offsets, sizes, iterations)
        return [flat_out[off:off + 3 * h * w].view(1, 3, h, w) for off, (h, w) in zip(offsets, sizes)]
    if not (torch.is_tensor(out) and torch.is_tensor(cond)) or out.shape != cond.shape or out.dim() not in (3, 4) \
            or out.shape[-3] != 3 or out.numel() == 0:
        raise ValueError("back_project_on_device: out and cond are [3,H,W] or [B,3,H,W] tensors of one shape")
    h, w = int(out.shape[-2]), int(out.shape[-1])
    check_hr_sizes([(h, w)])
    batch = 1 if out.dim() == 3 else int(out.shape[0])
    src = out.to(torch.float32).contiguous()
    dst = torch.empty_like(src)
    back_project_flat(src, cond.to(out.device, torch.float32).contiguous(), [i * 3 * h * w for i in range(batch)], [(h, w)] * batch,
                      iterations, dst=dst)
    return dst
