"""Quality numbers of a sampler output against its ground truth on the GPU (engine extension, absent upstream): Y-channel PSNR, RGB
PSNR and Y-channel SSIM with a border crop - ``srgd_image_metrics_images`` of ``libsrgd_metrics.so`` (srgd_amd/csrc/metrics.hip,
the arithmetic is fixed in include/srgd_metrics.h; a library of its own beside the engine's, built by the same srgd_amd/build.py).
There is no CPU path and no torch arithmetic here: torch allocates the results and the scratch, and one copy of ``4 * n`` doubles per call brings the numbers to the host."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib

TILE_H, TILE_W = 8, 32                  # SSIM positions per workgroup (metrics.hip: MX_TH, MX_TW)
WINDOW = 11
KEYS = ("psnr_y", "psnr_rgb", "ssim_y")
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsrgd_metrics.so")
# name -> (restype, argtypes); every symbol include/srgd_metrics.h declares
PROTOTYPES = {
    "srgd_image_metrics_last_error": (C.c_char_p, []),
    "srgd_image_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "srgd_image_metrics_images": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                            C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}
_handle = None


def lib() -> C.CDLL:
    """Load the metrics library (once).  Raises if it has not been built - no CPU fallback."""
    global _handle
    if _handle is None:
        _handle = _lib.load(LIB_PATH, PROTOTYPES, "The metrics run on the MI355X only")
    return _handle


def check_sizes(sizes, crop_border):
    """``ValueError`` unless ``crop_border`` >= 0 and every ``(h, w)`` keeps at least 11 x 11 pixels inside the crop."""
    if not isinstance(crop_border, int) or crop_border < 0:
        raise ValueError(f"metrics: crop_border must be an int >= 0, got {crop_border!r}")
    for (h, w) in sizes:
        if h - 2 * crop_border < WINDOW or w - 2 * crop_border < WINDOW:
            raise ValueError(f"metrics: a {h}x{w} image keeps fewer than {WINDOW}x{WINDOW} pixels inside a crop of {crop_border} "
                             "(no SSIM position)")


def scratch_doubles(sizes, crop_border):
    """float64 elements of the scratch buffer the C entry needs (include/srgd_metrics.h: four per 32x8 tile of SSIM positions)."""
    check_sizes(sizes, crop_border)
    up = lambda a, b: (a + b - 1) // b                  # noqa: E731
    return sum(4 * up(h - 2 * crop_border - (WINDOW - 1), TILE_H) * up(w - 2 * crop_border - (WINDOW - 1), TILE_W) for (h, w) in sizes)


def metrics_flat_device(out, ref_u8, out_offsets, ref_offsets, sizes, crop_border=4):
    """One batched call on flat device buffers; returns the device tensor ``[n, 4]`` float64 of (psnr_y, psnr_rgb, ssim_y,
    n_nonfinite) without synchronising.  ``out``: fp32, image i's ``[3,h_i,w_i]`` planes from element ``out_offsets[i]``;
    ``ref_u8``: uint8, its ``[h_i,w_i,3]`` bytes from byte ``ref_offsets[i]``."""
    if not (out.is_cuda and ref_u8.is_cuda):
        raise _lib.SrgdHipError("metrics run on MI355X only (no CPU fallback)")
    if out.dtype != torch.float32 or ref_u8.dtype != torch.uint8 or not out.is_contiguous() or not ref_u8.is_contiguous() \
            or out.device != ref_u8.device:
        raise ValueError("metrics: a contiguous fp32 output buffer and a contiguous uint8 reference buffer on one device")
    n = len(sizes)
    if len(out_offsets) != n or len(ref_offsets) != n:
        raise ValueError("metrics: one output offset and one reference offset per image")
    results = torch.empty(n, 4, device=out.device, dtype=torch.float64)
    if n == 0:
        return results
    sizes = [(int(h), int(w)) for (h, w) in sizes]
    n_scratch = scratch_doubles(sizes, crop_border)
    if min(out_offsets) < 0 or min(ref_offsets) < 0 \
            or max(o + 3 * h * w for o, (h, w) in zip(out_offsets, sizes)) > out.numel() \
            or max(o + 3 * h * w for o, (h, w) in zip(ref_offsets, sizes)) > ref_u8.numel():
        raise ValueError("metrics: offsets / sizes do not fit the buffers")
    scratch = torch.empty(n_scratch, device=out.device, dtype=torch.float64)
    o_offs = (C.c_int64 * n)(*out_offsets)
    r_offs = (C.c_int64 * n)(*ref_offsets)
    hw = (C.c_int32 * (2 * n))(*[v for size in sizes for v in size])
    with torch.cuda.device(out.device):
        rc = lib().srgd_image_metrics_images(C.c_void_p(out.data_ptr()), C.c_void_p(ref_u8.data_ptr()), o_offs, r_offs, hw, n, crop_border,
                                             C.c_void_p(results.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _lib.error_of(lib(), "srgd_image_metrics_last_error")
    return results


def records(results):
    """The device ``[n, 4]`` result of ``metrics_flat_device`` as a list of ``{"psnr_y", "psnr_rgb", "ssim_y"}`` dicts of Python
    floats: the one device-to-host copy of a group."""
    return [dict(zip(KEYS, row[:3])) for row in results.cpu().tolist()]


def metrics_flat(out, ref_u8, out_offsets, ref_offsets, sizes, crop_border=4):
    """``metrics_flat_device`` brought to the host: a list of ``{"psnr_y", "psnr_rgb", "ssim_y"}`` dicts of Python floats (``inf``
    for identical images, NaN where the output holds a non-finite value inside the crop)."""
    return records(metrics_flat_device(out, ref_u8, out_offsets, ref_offsets, sizes, crop_border))


def pack_references(reference, sizes, device):
    """``reference`` (a uint8 ``[H,W,3]`` tensor or a list of them, one per image of ``sizes``) as one flat uint8 device buffer and
    the images' byte offsets.  ``ValueError`` where count, dtype or shape do not fit."""
    refs = list(reference) if isinstance(reference, (list, tuple)) else [reference]
    if len(refs) != len(sizes):
        raise ValueError(f"metrics: {len(refs)} references for {len(sizes)} images")
    for r, (h, w) in zip(refs, sizes):
        if not torch.is_tensor(r) or r.dtype != torch.uint8 or tuple(r.shape) != (h, w, 3):
            raise ValueError(f"metrics: the reference of a {h}x{w} image is a uint8 [{h},{w},3] tensor")
    offsets, total = [], 0
    for (h, w) in sizes:
        offsets.append(total)
        total += 3 * h * w
    flat = torch.cat([r.to(device).reshape(-1) for r in refs]) if len(refs) > 1 else refs[0].to(device).contiguous().reshape(-1)
    return flat, offsets


def metrics_on_device(out, ref_u8, crop_border=4):
    """PSNR / SSIM of ``out`` (fp32 in [0,1] on the GPU) against ``ref_u8`` (uint8, height x width x 3):

    * a tensor ``[3,H,W]``, ``[1,3,H,W]`` or ``[B,3,H,W]`` with a reference ``[H,W,3]`` (B = 1), ``[B,H,W,3]`` or a list of B;
    * a list (tuple) of ``[1,3,H_i,W_i]`` tensors, sizes free, with a list of ``[H_i,W_i,3]`` references;

    every image in ONE batched call.  Returns a list of ``{"psnr_y", "psnr_rgb", "ssim_y"}`` dicts, one per image.
    ``ValueError``: shapes that do not match, an image smaller than 11 x 11 inside the crop."""
    if isinstance(out, (list, tuple)):
        if not out or not isinstance(ref_u8, (list, tuple)):
            raise ValueError("metrics_on_device: a list of outputs takes a list of references")
        for o in out:
            if not torch.is_tensor(o) or o.dim() != 4 or o.shape[0] != 1 or o.shape[1] != 3:
                raise ValueError("metrics_on_device: lists hold [1,3,H,W] outputs")
        dev = out[0].device
        sizes = [(int(o.shape[2]), int(o.shape[3])) for o in out]
        check_sizes(sizes, crop_border)
        refs, r_offs = pack_references(ref_u8, sizes, dev)
        flat = torch.cat([o.to(dev, torch.float32).reshape(-1) for o in out])
        return metrics_flat(flat, refs, r_offs, r_offs, sizes, crop_border)      # both layouts are 3 h w per image, packed
    if not torch.is_tensor(out) or out.dim() not in (3, 4) or out.shape[-3] != 3 or out.numel() == 0:
        raise ValueError("metrics_on_device: out is a [3,H,W] or [B,3,H,W] tensor, or a list of [1,3,H,W] tensors")
    h, w = int(out.shape[-2]), int(out.shape[-1])
    batch = 1 if out.dim() == 3 else int(out.shape[0])
    sizes = [(h, w)] * batch
    check_sizes(sizes, crop_border)
    if torch.is_tensor(ref_u8):
        ref_u8 = [ref_u8] if ref_u8.dim() == 3 else list(ref_u8)
    refs, r_offs = pack_references(ref_u8, sizes, out.device)
    return metrics_flat(out.to(torch.float32).contiguous().reshape(-1), refs, r_offs, r_offs, sizes, crop_border)
