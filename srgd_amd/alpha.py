"""Keeping the alpha channel of transparent inputs on the GPU (engine extension, absent upstream) - ``libsrgd_alpha.so``
(srgd_amd/csrc/alpha.hip, the definitions are fixed in include/srgd_alpha.h; a library of its own beside the eight others, built by
the same srgd_amd/build.py): a Pillow-exact resize of 8-bit planes (``Image.resize`` of an ``L`` image, which is band A of the
resize of an RGBA image, bit for bit), the interleave of an RGB image and a plane into RGBA, and the alpha bleed that spreads the
colours of visible pixels into the transparent area before the image is enlarged.  ``--alpha keep`` and ``--alpha_bleed N`` of the
folder driver use them.  The resize tables come from ``srgd_amd.resize.build_tables`` (the host function of libsrgd_resize.so:
Pillow's doubles stay in one place).  There is no CPU path and no torch arithmetic here: torch allocates the buffers, uploads the
tables and packs the images of a list; ``alpha_of`` alone runs on the host (it reads a decoded file)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from . import resize as RZ
from ._flat import ALIGN, check_flat, device_of, gather, layout, round16

MAX_SIDE = 16384
MAX_BLEED = 64
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsrgd_alpha.so")


class AlphaPlane(C.Structure):
    """``srgd_alpha_plane`` of include/srgd_alpha.h."""
    _fields_ = [("src_off", C.c_int64), ("dst_off", C.c_int64), ("tab_off", C.c_int64),
                ("h_in", C.c_int32), ("w_in", C.c_int32), ("h_out", C.c_int32), ("w_out", C.c_int32), ("k_h", C.c_int32), ("k_v", C.c_int32)]


class AlphaImage(C.Structure):
    """``srgd_alpha_image`` of include/srgd_alpha.h."""
    _fields_ = [("rgb_off", C.c_int64), ("a_off", C.c_int64), ("rgba_off", C.c_int64), ("h", C.c_int32), ("w", C.c_int32)]


# name -> (restype, argtypes); every symbol include/srgd_alpha.h declares
PROTOTYPES = {
    "srgd_alpha_last_error": (C.c_char_p, []),
    "srgd_alpha_resize_planes": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(AlphaPlane), C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_int64, C.c_void_p]),
    "srgd_alpha_pack_rgba": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AlphaImage), C.c_int, C.c_void_p]),
    "srgd_alpha_bleed": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(AlphaImage), C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
}
_handle = None


def lib() -> C.CDLL:
    """Load the alpha library (once).  Raises if it has not been built - no CPU fallback."""
    global _handle
    if _handle is None:
        _handle = _lib.load(LIB_PATH, PROTOTYPES, "The alpha kernels run on the MI355X only")
    return _handle


def _error():
    return _lib.error_of(lib(), "srgd_alpha_last_error")


def check_mode(mode):
    """``None`` -> "drop"; "drop" / "keep" -> itself; anything else raises ``ValueError``."""
    if mode is None:
        return "drop"
    if mode not in ("drop", "keep"):
        raise ValueError(f"alpha: mode must be drop or keep, got {mode!r}")
    return mode


def check_bleed(passes):
    """An integer in 0 .. 64 -> the int; anything else raises ``ValueError``."""
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or not 0 <= passes <= MAX_BLEED:
        raise ValueError(f"alpha_bleed: N must be an integer in 0 .. {MAX_BLEED}, got {passes!r}")
    return int(passes)


def alpha_of(pil_image):
    """The alpha plane of a decoded image (host): uint8 ``[h,w]`` = ``im.convert("RGBA").getchannel("A")`` where
    ``im.has_transparency_data`` (modes RGBA, LA, PA, and P / L / RGB with a tRNS chunk), ``None`` otherwise."""
    if not pil_image.has_transparency_data:
        return None
    return np.asarray(pil_image.convert("RGBA").getchannel("A"), dtype=np.uint8).copy()


def _check_hw(what, sizes):
    for h, w in sizes:
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"{what}: {h}x{w} is outside what the kernels take (sizes in 1 .. {MAX_SIDE})")


def plane_scratch_bytes(sizes):
    """Bytes of the scratch ``srgd_alpha_resize_planes`` needs for ``[(h_in, w_in, h_out, w_out)]``: per plane the horizontal pass's
    ``h_in * w_out`` bytes, rounded up to a multiple of 16."""
    return sum(round16(h_in * w_out) for (h_in, _, _, w_out) in sizes)


def bleed_scratch_bytes(sizes):
    """Bytes of the scratch ``srgd_alpha_bleed`` needs for ``[(h, w)]``: two state buffers of one dword per pixel, every image's
    part rounded up to a multiple of 16."""
    return 2 * sum(round16(4 * h * w) for h, w in sizes)


def resize_planes_flat(src, src_offsets, dst, dst_offsets, sizes, filter="bicubic"):
    """One batched call on flat uint8 device buffers: plane i's ``[h_in,w_in]`` bytes start at ``src_offsets[i]`` of ``src``, its
    result ``[h_out,w_out]`` at ``dst_offsets[i]`` of ``dst`` (offsets are multiples of 16), ``sizes`` = ``[(h_in, w_in, h_out,
    w_out)]``.  The tables come from ``srgd_amd.resize.build_tables`` and are uploaded; the scratch is allocated here.  Returns
    ``dst``.  No synchronisation."""
    filter = RZ.check_filter(filter)
    sizes = [tuple(int(v) for v in size) for size in sizes]
    n = len(sizes)
    RZ.check_sizes(sizes)
    check_flat("alpha plane resize", (src, dst), n, (src, src_offsets, [s[0] * s[1] for s in sizes]),
                (dst, dst_offsets, [s[2] * s[3] for s in sizes]))
    host_tables, tab_offsets = RZ.build_tables(sizes, filter)
    tables = torch.from_numpy(np.concatenate([host_tables, np.zeros(4, np.int32)])).to(src.device)       # never empty
    scratch = torch.empty(max(plane_scratch_bytes(sizes), ALIGN), device=src.device, dtype=torch.uint8)
    planes = (AlphaPlane * n)(*[AlphaPlane(so, do, to, h_in, w_in, h_out, w_out,
                                           RZ.ksize(w_in, w_out, filter) if w_in != w_out else 0,
                                           RZ.ksize(h_in, h_out, filter) if h_in != h_out else 0)
                                for so, do, to, (h_in, w_in, h_out, w_out) in zip(src_offsets, dst_offsets, tab_offsets, sizes)])
    with torch.cuda.device(src.device):
        rc = lib().srgd_alpha_resize_planes(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), planes, n,
                                            C.c_void_p(tables.data_ptr()), 4 * tables.numel(), C.c_void_p(scratch.data_ptr()),
                                            scratch.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _error()
    return dst


def pack_rgba_flat(rgb, rgb_offsets, alpha, alpha_offsets, rgba, rgba_offsets, sizes):
    """One batched call on flat uint8 device buffers: image i's ``[h,w,3]`` colour at ``rgb_offsets[i]`` of ``rgb`` and its ``[h,w]``
    plane at ``alpha_offsets[i]`` of ``alpha`` -> ``[h,w,4]`` at ``rgba_offsets[i]`` of ``rgba``; ``sizes`` = ``[(h, w)]``.  Returns
    ``rgba``.  No synchronisation."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    n = len(sizes)
    _check_hw("alpha pack", sizes)
    check_flat("alpha pack", (rgb, alpha, rgba), n, (rgb, rgb_offsets, [3 * h * w for h, w in sizes]),
                (alpha, alpha_offsets, [h * w for h, w in sizes]), (rgba, rgba_offsets, [4 * h * w for h, w in sizes]))
    images = (AlphaImage * n)(*[AlphaImage(co, ao, do, h, w) for co, ao, do, (h, w) in zip(rgb_offsets, alpha_offsets, rgba_offsets, sizes)])
    with torch.cuda.device(rgb.device):
        rc = lib().srgd_alpha_pack_rgba(C.c_void_p(rgb.data_ptr()), C.c_void_p(alpha.data_ptr()), C.c_void_p(rgba.data_ptr()), images, n,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _error()
    return rgba


def bleed_flat(rgba, rgba_offsets, rgb, rgb_offsets, sizes, passes):
    """One batched call on flat uint8 device buffers: image i's ``[h,w,4]`` pixels at ``rgba_offsets[i]`` of ``rgba`` -> its bled
    ``[h,w,3]`` colour at ``rgb_offsets[i]`` of ``rgb`` after ``passes`` passes; ``sizes`` = ``[(h, w)]``.  The scratch is allocated
    here.  Returns ``rgb``.  No synchronisation."""
    passes = check_bleed(passes)
    sizes = [(int(h), int(w)) for h, w in sizes]
    n = len(sizes)
    _check_hw("alpha bleed", sizes)
    check_flat("alpha bleed", (rgba, rgb), n, (rgba, rgba_offsets, [4 * h * w for h, w in sizes]),
                (rgb, rgb_offsets, [3 * h * w for h, w in sizes]))
    scratch = torch.empty(max(bleed_scratch_bytes(sizes) if passes else 0, ALIGN), device=rgba.device, dtype=torch.uint8)
    images = (AlphaImage * n)(*[AlphaImage(do, 0, so, h, w) for so, do, (h, w) in zip(rgba_offsets, rgb_offsets, sizes)])
    with torch.cuda.device(rgba.device):
        rc = lib().srgd_alpha_bleed(C.c_void_p(rgba.data_ptr()), C.c_void_p(rgb.data_ptr()), images, n, passes,
                                    C.c_void_p(scratch.data_ptr()), scratch.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _error()
    return rgb


def _check_list(what, tensors, channels):
    """A non-empty list of uint8 tensors ``[H,W,channels]`` (``[H,W]`` for channels None)."""
    if not isinstance(tensors, (list, tuple)) or not tensors:
        raise ValueError(f"{what}: a non-empty list of tensors")
    for t in tensors:
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != (2 if channels is None else 3) \
                or (channels is not None and t.shape[2] != channels):
            raise ValueError(f"{what}: uint8 [H,W{'' if channels is None else ',' + str(channels)}] tensors")
    _check_hw(what, [(int(t.shape[0]), int(t.shape[1])) for t in tensors])


def bleed_on_device(rgba_list, passes):
    """``rgba_list``: uint8 ``[h_i,w_i,4]`` tensors (moved to the GPU if they are not there) -> a list of uint8 ``[h_i,w_i,3]`` device
    tensors: the colour after ``passes`` (0 .. 64) passes of the alpha bleed of include/srgd_alpha.h; every image in ONE batched
    call.  ``ValueError``: shapes that are not ``[H,W,4]`` uint8, passes outside 0 .. 64."""
    passes = check_bleed(passes)
    _check_list("bleed_on_device", rgba_list, 4)
    dev = device_of(rgba_list, "the alpha bleed")
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in rgba_list]
    src, src_offsets = gather(rgba_list, dev)
    dst_offsets, total = layout([3 * h * w for h, w in sizes])
    dst = torch.empty(total, device=dev, dtype=torch.uint8)
    bleed_flat(src, src_offsets, dst, dst_offsets, sizes, passes)
    return [dst[off:off + 3 * h * w].view(h, w, 3) for off, (h, w) in zip(dst_offsets, sizes)]


def resize_planes_on_device(planes, sizes, filter="bicubic"):
    """``planes``: uint8 ``[H_i,W_i]`` tensors (moved to the GPU if they are not there), ``sizes``: one ``(h_out, w_out)`` per plane
    -> a list of uint8 ``[h_out,w_out]`` device tensors, ``Image.resize((w_out, h_out), filter)`` of each as an ``L`` image bit for
    bit; every plane in ONE batched call.  ``ValueError``: an unknown filter, shapes that are not ``[H,W]`` uint8, a size outside
    1 .. 16384 or a ratio above 8."""
    filter = RZ.check_filter(filter)
    _check_list("resize_planes_on_device", planes, None)
    if len(planes) != len(sizes):
        raise ValueError("resize_planes_on_device: one (h_out, w_out) per plane")
    geo = [(int(p.shape[0]), int(p.shape[1]), int(h), int(w)) for p, (h, w) in zip(planes, sizes)]
    RZ.check_sizes(geo)
    dev = device_of(planes, "the alpha plane resize")
    src, src_offsets = gather(planes, dev)
    dst_offsets, total = layout([h * w for (_, _, h, w) in geo])
    dst = torch.empty(total, device=dev, dtype=torch.uint8)
    resize_planes_flat(src, src_offsets, dst, dst_offsets, geo, filter)
    return [dst[off:off + h * w].view(h, w) for off, (_, _, h, w) in zip(dst_offsets, geo)]


def pack_rgba_on_device(rgb_list, alpha_list):
    """``rgb_list``: uint8 ``[H_i,W_i,3]`` tensors, ``alpha_list``: uint8 ``[H_i,W_i]`` tensors (moved to the GPU if they are not
    there) -> a list of uint8 ``[H_i,W_i,4]`` device tensors, ``Image.merge("RGBA", (*rgb.split(), alpha))`` of each; ONE call."""
    _check_list("pack_rgba_on_device", rgb_list, 3)
    _check_list("pack_rgba_on_device", alpha_list, None)
    if len(rgb_list) != len(alpha_list) or any(tuple(c.shape[:2]) != tuple(a.shape) for c, a in zip(rgb_list, alpha_list)):
        raise ValueError("pack_rgba_on_device: one [H,W] plane per [H,W,3] image")
    dev = device_of(list(rgb_list) + list(alpha_list), "the alpha pack")
    sizes = [(int(c.shape[0]), int(c.shape[1])) for c in rgb_list]
    rgb, rgb_offsets = gather(rgb_list, dev)
    alpha, alpha_offsets = gather(alpha_list, dev)
    dst_offsets, total = layout([4 * h * w for h, w in sizes])
    dst = torch.empty(total, device=dev, dtype=torch.uint8)
    pack_rgba_flat(rgb, rgb_offsets, alpha, alpha_offsets, dst, dst_offsets, sizes)
    return [dst[off:off + 4 * h * w].view(h, w, 4) for off, (h, w) in zip(dst_offsets, sizes)]


def attach_alpha_on_device(rgb_list, alpha_lr_list, scale=4, filter="bicubic"):
    """What ``--alpha keep`` writes: ``rgb_list`` uint8 ``[H_i,W_i,3]`` outputs, ``alpha_lr_list`` the uint8 ``[h_i,w_i]`` alpha
    planes of their inputs -> a list of uint8 ``[H_i,W_i,4]`` device tensors.  Every plane is enlarged x``scale`` with Pillow's
    bicubic (the operator that makes the model's conditions); where an output is not x``scale`` of its plane (``--outscale``) that
    plane is resized again to the output's size with ``filter`` - the alpha band Pillow's ``Image.resize`` gives for the RGBA image
    built at x``scale``; then colour and alpha are interleaved.  One batched call per stage.  The colour is not premultiplied."""
    filter = RZ.check_filter(filter)
    _check_list("attach_alpha_on_device", rgb_list, 3)
    _check_list("attach_alpha_on_device", alpha_lr_list, None)
    if len(rgb_list) != len(alpha_lr_list) or isinstance(scale, bool) or not isinstance(scale, int) or not 1 <= scale <= RZ.MAX_RATIO:
        raise ValueError("attach_alpha_on_device: one plane per image and an integer scale in 1 .. 8")
    up = [(scale * int(a.shape[0]), scale * int(a.shape[1])) for a in alpha_lr_list]
    final = [(int(c.shape[0]), int(c.shape[1])) for c in rgb_list]
    RZ.check_sizes([(int(a.shape[0]), int(a.shape[1])) + s for a, s in zip(alpha_lr_list, up)])
    RZ.check_sizes([s + f for s, f in zip(up, final)])
    planes = resize_planes_on_device(alpha_lr_list, up, "bicubic")
    again = [i for i in range(len(planes)) if up[i] != final[i]]
    if again:
        for i, p in zip(again, resize_planes_on_device([planes[i] for i in again], [final[i] for i in again], filter)):
            planes[i] = p
    return pack_rgba_on_device(rgb_list, planes)
