"""Mean image and spread map of the K samples of an image on the GPU (engine extension, absent upstream) -
``srgd_image_ensemble_images`` of ``libsrgd_ensemble.so`` (srgd_amd/csrc/ensemble.hip, the arithmetic is fixed in
include/srgd_ensemble.h; a library of its own beside the engine's and the metrics', built by the same srgd_amd/build.py).
The inputs are uint8 samples as saved; every output but ``mean_std`` is an exact function of integers.
There is no CPU path and no torch arithmetic here: torch allocates the buffers and copies the samples into the padded layout, and one
copy of ``2 * n`` doubles per call brings the statistics to the host."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib

VEC = 16                                # bytes of a lane per sample: sample strides and offsets are multiples of it (ensemble.hip: EN_VEC)
CHUNK = 4096                            # elements per {sum, max} record of the scratch (ensemble.hip: EN_CHUNK)
MIN_SAMPLES, MAX_SAMPLES = 2, 256
KEYS = ("mean_std", "max_std")
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsrgd_ensemble.so")
# name -> (restype, argtypes); every symbol include/srgd_ensemble.h declares
PROTOTYPES = {
    "srgd_image_ensemble_last_error": (C.c_char_p, []),
    "srgd_image_ensemble": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "srgd_image_ensemble_images": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
}
_handle = None


def lib() -> C.CDLL:
    """Load the ensemble library (once).  Raises if it has not been built - no CPU fallback."""
    global _handle
    if _handle is None:
        _handle = _lib.load(LIB_PATH, PROTOTYPES, "The ensemble runs on the MI355X only")
    return _handle


def padded(n):
    """``n`` rounded up to a multiple of 16: the stride between the samples of an image of ``n`` bytes."""
    return (n + VEC - 1) // VEC * VEC


def scratch_doubles(sizes):
    """float64 elements of the scratch buffer the C entry needs (include/srgd_ensemble.h: two 8-byte words per chunk of 4096
    elements)."""
    for (h, w) in sizes:
        if h < 1 or w < 1:
            raise ValueError(f"ensemble: bad image size {h}x{w}")
    return sum(2 * ((3 * h * w + CHUNK - 1) // CHUNK) for (h, w) in sizes)


def ensemble_flat_device(samples, sample_offsets, sizes, n_samples, mean_u8, std_u8, out_offsets, mean01=None, mean01_offsets=None):
    """One batched call on flat device buffers; returns the device tensor ``[n, 2]`` float64 of (mean_std, max_std) without
    synchronising.  ``samples``: uint8, sample k of image i is ``[h_i,w_i,3]`` from byte ``sample_offsets[i] + k * padded(3 h_i w_i)``;
    ``mean_u8`` / ``std_u8``: uint8, image i's ``[h_i,w_i,3]`` outputs from byte ``out_offsets[i]`` of each; ``mean01`` (optional):
    fp32, its ``[3,h_i,w_i]`` planes from element ``mean01_offsets[i]``.  Sample and output offsets are multiples of 16."""
    if not (samples.is_cuda and mean_u8.is_cuda and std_u8.is_cuda):
        raise _lib.SrgdHipError("the ensemble runs on MI355X only (no CPU fallback)")
    bufs = [samples, mean_u8, std_u8] + ([mean01] if mean01 is not None else [])
    if any(b.dtype != torch.uint8 for b in bufs[:3]) or (mean01 is not None and mean01.dtype != torch.float32) \
            or any(not b.is_contiguous() or b.device != samples.device for b in bufs):
        raise ValueError("ensemble: contiguous uint8 sample, mean and spread buffers (and an fp32 mean01 buffer) on one device")
    if (mean01 is None) != (mean01_offsets is None):
        raise ValueError("ensemble: mean01 and its offsets are given together")
    n = len(sizes)
    if n < 1 or len(sample_offsets) != n or len(out_offsets) != n or (mean01_offsets is not None and len(mean01_offsets) != n):
        raise ValueError("ensemble: at least one image, and one sample offset and one output offset per image")
    if not isinstance(n_samples, int) or not MIN_SAMPLES <= n_samples <= MAX_SAMPLES:
        raise ValueError(f"ensemble: the number of samples must be in {MIN_SAMPLES}..{MAX_SAMPLES}, got {n_samples!r}")
    sizes = [(int(h), int(w)) for (h, w) in sizes]
    n_scratch = scratch_doubles(sizes)
    elems = [3 * h * w for (h, w) in sizes]
    if min(sample_offsets) < 0 or min(out_offsets) < 0 \
            or max(o + (n_samples - 1) * padded(e) + e for o, e in zip(sample_offsets, elems)) > samples.numel() \
            or max(o + e for o, e in zip(out_offsets, elems)) > min(mean_u8.numel(), std_u8.numel()) \
            or (mean01 is not None and (min(mean01_offsets) < 0 or max(o + e for o, e in zip(mean01_offsets, elems)) > mean01.numel())):
        raise ValueError("ensemble: offsets / sizes do not fit the buffers")
    stats = torch.empty(n, 2, device=samples.device, dtype=torch.float64)
    scratch = torch.empty(n_scratch, device=samples.device, dtype=torch.float64)
    s_offs = (C.c_int64 * n)(*sample_offsets)
    o_offs = (C.c_int64 * n)(*out_offsets)
    m_offs = (C.c_int64 * n)(*mean01_offsets) if mean01 is not None else None
    hw = (C.c_int32 * (2 * n))(*[v for size in sizes for v in size])
    with torch.cuda.device(samples.device):
        rc = lib().srgd_image_ensemble_images(C.c_void_p(samples.data_ptr()), s_offs, hw, n, n_samples, C.c_void_p(mean_u8.data_ptr()),
                                              C.c_void_p(std_u8.data_ptr()), o_offs,
                                              C.c_void_p(mean01.data_ptr()) if mean01 is not None else None, m_offs,
                                              C.c_void_p(stats.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _lib.error_of(lib(), "srgd_image_ensemble_last_error")
    return stats


def records(stats):
    """The device ``[n, 2]`` result of ``ensemble_flat_device`` as a list of ``{"mean_std", "max_std"}`` dicts of Python floats: the
    one device-to-host copy of a group."""
    return [dict(zip(KEYS, row)) for row in stats.cpu().tolist()]


def ensemble_flat(samples, sample_offsets, sizes, n_samples, mean_u8, std_u8, out_offsets, mean01=None, mean01_offsets=None):
    """``ensemble_flat_device`` brought to the host: a list of ``{"mean_std", "max_std"}`` dicts of Python floats in 8-bit units."""
    return records(ensemble_flat_device(samples, sample_offsets, sizes, n_samples, mean_u8, std_u8, out_offsets, mean01, mean01_offsets))


def ensemble_on_device(samples, return_mean01=False):
    """Mean image and spread map of the K samples of every image: ``samples`` is a uint8 ``[K,H,W,3]`` tensor on the GPU, or a list
    (tuple) of such tensors, sizes free, one K (2..256) - every image of a list in ONE batched call.  Returns, per image,
    ``(mean_u8 [H,W,3], std_u8 [H,W,3], {"mean_std", "max_std"})`` - one tuple for a tensor, a list of them for a list - with
    ``mean01 [1,3,H,W]`` (fp32, the mean image as ``ToTensor`` reads it back) as a fourth item where ``return_mean01`` is set.
    The samples are copied into the padded layout of the C entry here.  ``ValueError``: shapes or dtypes that do not fit."""
    single = torch.is_tensor(samples)
    images = [samples] if single else (list(samples) if isinstance(samples, (list, tuple)) else None)
    if not images:
        raise ValueError("ensemble_on_device: a uint8 [K,H,W,3] tensor or a non-empty list of them")
    for t in images:
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or t.numel() == 0:
            raise ValueError("ensemble_on_device: every image is a uint8 [K,H,W,3] tensor of its K samples")
    k = int(images[0].shape[0])
    if any(int(t.shape[0]) != k for t in images) or not MIN_SAMPLES <= k <= MAX_SAMPLES:
        raise ValueError(f"ensemble_on_device: one K in {MIN_SAMPLES}..{MAX_SAMPLES} for all images")
    dev = images[0].device
    if not all(t.is_cuda and t.device == dev for t in images):
        raise _lib.SrgdHipError("the ensemble runs on MI355X only (no CPU fallback): the samples are tensors of one GPU")
    sizes = [(int(t.shape[1]), int(t.shape[2])) for t in images]
    elems = [3 * h * w for (h, w) in sizes]
    s_offs, o_offs, m_offs, s_total, o_total, m_total = [], [], [], 0, 0, 0
    for e in elems:
        s_offs.append(s_total)
        o_offs.append(o_total)
        m_offs.append(m_total)
        s_total += k * padded(e)
        o_total += padded(e)
        m_total += e
    flat = torch.empty(s_total, device=dev, dtype=torch.uint8)
    for t, off, e in zip(images, s_offs, elems):         # one strided copy per image; the padding stays as it is and is never read
        flat[off:off + k * padded(e)].view(k, padded(e))[:, :e].copy_(t.reshape(k, e))
    mean = torch.empty(o_total, device=dev, dtype=torch.uint8)
    std = torch.empty(o_total, device=dev, dtype=torch.uint8)
    m01 = torch.empty(m_total, device=dev, dtype=torch.float32) if return_mean01 else None
    stats = ensemble_flat(flat, s_offs, sizes, k, mean, std, o_offs, m01, m_offs if return_mean01 else None)
    out = []
    for i, ((h, w), e) in enumerate(zip(sizes, elems)):
        item = (mean[o_offs[i]:o_offs[i] + e].view(h, w, 3), std[o_offs[i]:o_offs[i] + e].view(h, w, 3), stats[i])
        if return_mean01:
            item += (m01[m_offs[i]:m_offs[i] + e].view(1, 3, h, w),)
        out.append(item)
    return out[0] if single else out
