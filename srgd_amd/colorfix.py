"""Colour correction of a sampler output against its x4 bicubic condition on the GPU (engine extension, absent upstream):
``srgd_image_color_fix_images`` of ``libsrgd_hip.so`` - StableSR's ``wavelet_reconstruction`` / ``adaptive_instance_normalization``
arithmetic as HIP kernels (srgd_amd/csrc/imageio.hip, contract in include/srgd_hip.h).  There is no CPU path and no torch arithmetic
here: torch only allocates the result and the scratch."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

MODES = {"wavelet": 1, "adain": 2}
_ADAIN_CHUNK = 4096                     # pixels per float64 partial sum (imageio.hip: CF_CHUNK)


def check_mode(mode):
    """``None`` / ``"none"`` -> None (no correction); a known mode -> itself; anything else raises ``ValueError``."""
    if mode is None or mode == "none":
        return None
    if mode not in MODES:
        raise ValueError(f"color_fix: unknown mode {mode!r} (None, 'none', 'wavelet' or 'adain')")
    return mode


def scratch_elements(mode, offsets, sizes):
    """fp32 elements of the scratch buffer the C entry needs (include/srgd_hip.h states the two formulas)."""
    if mode == "wavelet":
        extent = max(off + 3 * h * w for off, (h, w) in zip(offsets, sizes))
        return 2 * ((extent + 3) // 4 * 4)
    return sum(96 * (1 + (h * w + _ADAIN_CHUNK - 1) // _ADAIN_CHUNK) for (h, w) in sizes) // 4


def color_fix_flat(out, cond, offsets, sizes, mode, dst=None):
    """One batched call on flat fp32 device buffers: image i's ``[3,h_i,w_i]`` planes start at ``offsets[i]`` of ``out``, ``cond``
    and ``dst`` alike (``dst=None``: in place, the result replaces ``out``).  Returns ``dst``."""
    mode = check_mode(mode)
    if mode is None:
        raise ValueError("color_fix_flat needs a mode ('wavelet' or 'adain')")
    if not (out.is_cuda and cond.is_cuda):
        raise _lib.SrgdHipError("colour fix runs on MI355X only (no CPU fallback)")
    dst = out if dst is None else dst
    for t in (out, cond, dst):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != out.device:
            raise ValueError("color_fix: contiguous fp32 buffers on one device")
    n = len(sizes)
    end = max(off + 3 * h * w for off, (h, w) in zip(offsets, sizes))
    if len(offsets) != n or n < 1 or min(offsets) < 0 or end > min(out.numel(), cond.numel(), dst.numel()):
        raise ValueError("color_fix: offsets / sizes do not fit the buffers")
    scratch = torch.empty(scratch_elements(mode, offsets, sizes), device=out.device, dtype=torch.float32)
    offs = (C.c_int64 * n)(*offsets)
    hw = (C.c_int32 * (2 * n))(*[v for size in sizes for v in size])
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().srgd_image_color_fix_images(C.c_void_p(out.data_ptr()), C.c_void_p(cond.data_ptr()), offs, hw, n,
                                                         MODES[mode], C.c_void_p(dst.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "srgd_image_color_fix_images")
    return dst


def color_fix_on_device(out, cond, mode):
    """``out`` corrected against ``cond`` (``mode``: ``"wavelet"`` or ``"adain"``), both fp32 in [0,1] on the GPU:

    * tensors ``[3,H,W]``, ``[1,3,H,W]`` or ``[B,3,H,W]`` of one shape -> a new tensor of that shape;
    * lists (tuples) of ``[1,3,H_i,W_i]`` tensors, sizes free -> a list of new ``[1,3,H_i,W_i]`` tensors;

    every image in ONE batched call (the images of a list are packed into flat buffers first).  ``out`` is left as it is.
    ``ValueError``: unknown mode, shapes that do not match."""
    if check_mode(mode) is None:
        raise ValueError(f"color_fix_on_device: unknown mode {mode!r} ('wavelet' or 'adain')")
    if isinstance(out, (list, tuple)) != isinstance(cond, (list, tuple)):
        raise ValueError("color_fix_on_device: out and cond are both tensors or both lists")
    if isinstance(out, (list, tuple)):
        if len(out) != len(cond) or not out:
            raise ValueError("color_fix_on_device: one condition per output")
        for o, c in zip(out, cond):
            if not (torch.is_tensor(o) and torch.is_tensor(c)) or o.dim() != 4 or o.shape[0] != 1 or o.shape[1] != 3 \
                    or o.shape != c.shape:
                raise ValueError("color_fix_on_device: lists hold matching [1,3,H,W] tensors")
        dev = out[0].device
        sizes = [(int(o.shape[2]), int(o.shape[3])) for o in out]
        offsets, total = [], 0
        for (h, w) in sizes:
            offsets.append(total)
            total += 3 * h * w
        flat_out = torch.cat([o.to(dev, torch.float32).reshape(-1) for o in out])
        flat_cond = torch.cat([c.to(dev, torch.float32).reshape(-1) for c in cond])
        color_fix_flat(flat_out, flat_cond, offsets, sizes, mode)
        return [flat_out[off:off + 3 * h * w].view(1, 3, h, w) for off, (h, w) in zip(offsets, sizes)]
    if not (torch.is_tensor(out) and torch.is_tensor(cond)) or out.shape != cond.shape or out.dim() not in (3, 4) \
            or out.shape[-3] != 3 or out.numel() == 0:
        raise ValueError("color_fix_on_device: out and cond are [3,H,W] or [B,3,H,W] tensors of one shape")
    h, w = int(out.shape[-2]), int(out.shape[-1])
    batch = 1 if out.dim() == 3 else int(out.shape[0])
    src = out.to(torch.float32).contiguous()
    dst = torch.empty_like(src)
    color_fix_flat(src, cond.to(out.device, torch.float32).contiguous(), [i * 3 * h * w for i in range(batch)], [(h, w)] * batch,
                   mode, dst=dst)
    return dst
