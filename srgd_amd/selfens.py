"""Geometric self-ensemble on the GPU (engine extension, absent upstream) - ``libsrgd_selfens.so`` (srgd_amd/csrc/selfens.hip, the
definitions are fixed in include/srgd_selfens.h; a library of its own beside the ten others, built by the same srgd_amd/build.py):
the eight dihedral operations (flips / rotations) on 8-bit RGB images, and the fused merge that turns up to eight sources back and
averages them, halves up.  ``--self_ensemble N`` of the folder driver uses them: the model runs on ``OPS[N]`` of every input and the
outputs are merged.  There is no CPU path and no torch arithmetic here: torch allocates the buffers and packs the images of a list."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib
from ._flat import check_flat, gather, layout

MAX_SOURCES = 8                                           # SRGD_SELFENS_MAX_SOURCES
MAX_IMAGES = 32                                           # SRGD_SELFENS_MAX_IMAGES: images of one launch
TILE = 32                                                 # SRGD_SELFENS_TILE
LDS_TRANSFORM, LDS_MERGE = 3712, 32768                    # SRGD_SELFENS_LDS_TRANSFORM, SRGD_SELFENS_LDS_MERGE
# --self_ensemble N -> the ops of its variants, in the order the driver runs them: 2 adds the mirror image, 4 the four flips, 8 all
OPS = {1: (0,), 2: (0, 1), 4: (0, 1, 2, 3), 8: (0, 1, 2, 3, 4, 5, 6, 7)}
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsrgd_selfens.so")


class SelfensRecord(C.Structure):
    """``srgd_selfens_record`` of include/srgd_selfens.h."""
    _fields_ = [("src_off", C.c_int64), ("dst_off", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("op", C.c_int32), ("pad", C.c_int32)]


class SelfensImage(C.Structure):
    """``srgd_selfens_image`` of include/srgd_selfens.h."""
    _fields_ = [("dst_off", C.c_int64), ("mean01_off", C.c_int64), ("H", C.c_int32), ("W", C.c_int32), ("n_src", C.c_int32),
                ("pad", C.c_int32), ("src_off", C.c_int64 * 8), ("op", C.c_int32 * 8)]


# name -> (restype, argtypes); every symbol include/srgd_selfens.h declares
PROTOTYPES = {
    "srgd_selfens_last_error": (C.c_char_p, []),
    "srgd_selfens_transform": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SelfensRecord), C.c_int, C.c_void_p]),
    "srgd_selfens_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SelfensImage), C.c_int, C.c_void_p]),
}
_handle = None


def lib() -> C.CDLL:
    """Load the self-ensemble library (once).  Raises if it has not been built - no CPU fallback."""
    global _handle
    if _handle is None:
        _handle = _lib.load(LIB_PATH, PROTOTYPES, "The self-ensemble kernels run on the MI355X only")
    return _handle


def _error():
    return _lib.error_of(lib(), "srgd_selfens_last_error")


def check_self_ensemble(n):
    """``None`` / 1 -> 1 (off); 2, 4, 8 -> the int; anything else raises ``ValueError``."""
    if n is None:
        return 1
    if isinstance(n, bool) or not isinstance(n, int) or n not in OPS:
        raise ValueError(f"self_ensemble: N must be 1, 2, 4 or 8, got {n!r}")
    return n


def check_op(op):
    if isinstance(op, bool) or not isinstance(op, int) or not 0 <= op <= 7:
        raise ValueError(f"self-ensemble: an op is an integer in 0 .. 7, got {op!r}")
    return op


def inverse(op):
    """The op that undoes ``op``: ``apply(apply(x, op), inverse(op)) == x``.  Ops 5 and 6 (the two quarter turns) undo each other,
    every other op undoes itself."""
    return {5: 6, 6: 5}.get(check_op(op), op)


def out_size(h, w, op):
    """``(h, w)`` of ``apply`` of an ``[h,w,3]`` image."""
    return (w, h) if check_op(op) & 4 else (h, w)


def _check_hw(what, sizes):
    for h, w in sizes:
        if h < 1 or w < 1 or 3 * h * w >= 2 ** 31:
            raise ValueError(f"{what}: {h}x{w} is outside what the kernels take (sizes >= 1, 3*h*w < 2^31)")


def transform_flat(src, src_offsets, dst, dst_offsets, sizes, ops):
    """One batched call on caller-owned flat uint8 device buffers: image i's ``[h,w,3]`` bytes start at ``src_offsets[i]`` of
    ``src``, ``apply(image, ops[i])`` is written from ``dst_offsets[i]`` of ``dst`` (offsets are multiples of 16); ``sizes`` =
    ``[(h, w)]`` of the sources.  Returns ``dst``.  No synchronisation."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    ops = [check_op(op) for op in ops]
    n = len(sizes)
    if len(ops) != n or len(src_offsets) != n or len(dst_offsets) != n:
        raise ValueError("self-ensemble transform: one op, one source offset and one destination offset per image")
    _check_hw("self-ensemble transform", sizes)
    nbytes = [3 * h * w for h, w in sizes]
    check_flat("the self-ensemble transform", (src, dst), n, (src, src_offsets, nbytes), (dst, dst_offsets, nbytes))
    recs = (SelfensRecord * n)(*[SelfensRecord(so, do, h, w, op, 0) for so, do, (h, w), op in zip(src_offsets, dst_offsets, sizes, ops)])
    with torch.cuda.device(src.device):
        rc = lib().srgd_selfens_transform(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), recs, n,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _error()
    return dst


def merge_flat(src, src_offsets, ops, dst, dst_offsets, sizes, mean01=None, mean01_offsets=None):
    """One batched call on caller-owned flat device buffers: image i, ``sizes[i]`` = ``(H, W)``, has the sources ``src_offsets[i]``
    (a list of byte offsets into ``src``, multiples of 16) with the ops ``ops[i]``; source j is ``[H,W,3]`` for ``ops[i][j] < 4`` and
    ``[W,H,3]`` otherwise.  The merged ``[H,W,3]`` goes to ``dst_offsets[i]`` of ``dst``, its fp32 planes ``[3,H,W]`` to element
    ``mean01_offsets[i]`` of ``mean01`` where that is given.  Returns ``dst``.  No synchronisation."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    n = len(sizes)
    if len(ops) != n or len(src_offsets) != n or len(dst_offsets) != n or (mean01 is None) != (mean01_offsets is None) \
            or (mean01_offsets is not None and len(mean01_offsets) != n):
        raise ValueError("self-ensemble merge: one source list, one op list and one destination offset per image; mean01 and its "
                         "offsets are given together")
    ops = [[check_op(op) for op in image_ops] for image_ops in ops]
    if any(not 1 <= len(o) <= MAX_SOURCES or len(o) != len(s) for o, s in zip(ops, src_offsets)):
        raise ValueError(f"self-ensemble merge: 1 .. {MAX_SOURCES} sources per image, one op per source")
    _check_hw("self-ensemble merge", sizes)
    nbytes = [3 * h * w for h, w in sizes]
    check_flat("the self-ensemble merge", (src, dst), n, (src, [o for s in src_offsets for o in s], [b for s, b in zip(src_offsets, nbytes) for _ in s]),
                (dst, dst_offsets, nbytes))
    if mean01 is not None:
        if not mean01.is_cuda or mean01.dtype != torch.float32 or not mean01.is_contiguous() or mean01.device != src.device \
                or min(mean01_offsets) < 0 or max(o + b for o, b in zip(mean01_offsets, nbytes)) > mean01.numel():
            raise ValueError("self-ensemble merge: a contiguous fp32 mean01 buffer on the same device that holds every image's planes")
    images = (SelfensImage * n)()
    for i, ((h, w), offs, image_ops) in enumerate(zip(sizes, src_offsets, ops)):
        images[i].dst_off, images[i].mean01_off = dst_offsets[i], mean01_offsets[i] if mean01 is not None else 0
        images[i].H, images[i].W, images[i].n_src = h, w, len(offs)
        for j, (off, op) in enumerate(zip(offs, image_ops)):
            images[i].src_off[j], images[i].op[j] = off, op
    with torch.cuda.device(src.device):
        rc = lib().srgd_selfens_merge(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                                      C.c_void_p(mean01.data_ptr()) if mean01 is not None else None, images, n,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise _error()
    return dst


def _check_images(what, tensors):
    for t in tensors:
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.numel() == 0:
            raise ValueError(f"{what}: uint8 [H,W,3] tensors")
    _check_hw(what, [(int(t.shape[0]), int(t.shape[1])) for t in tensors])


def _one_gpu(what, tensors):
    dev = tensors[0].device
    if not all(t.is_cuda and t.device == dev for t in tensors):
        raise _lib.SrgdHipError(f"{what} runs on MI355X only (no CPU fallback): the images are tensors of one GPU")
    return dev


def dihedral_on_device(images, ops):
    """``images``: a list of uint8 ``[h_i,w_i,3]`` GPU tensors, ``ops``: one op (0 .. 7) per image -> a list of uint8 device tensors,
    ``apply(image, op)`` of include/srgd_selfens.h (``[w_i,h_i,3]`` for op >= 4); every image in ONE batched call.  An image may
    appear several times.  ``ValueError``: shapes, dtypes or ops that do not fit; CPU tensors: ``SrgdHipError``."""
    if not isinstance(images, (list, tuple)) or not images or not isinstance(ops, (list, tuple)) or len(ops) != len(images):
        raise ValueError("dihedral_on_device: a non-empty list of images and one op per image")
    _check_images("dihedral_on_device", images)
    ops = [check_op(op) for op in ops]
    dev = _one_gpu("the self-ensemble transform", images)
    unique = {}
    for t in images:
        unique.setdefault(id(t), t)
    src, offs = gather(list(unique.values()), dev)
    where = dict(zip(unique, offs))
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in images]
    dst_offsets, total = layout([3 * h * w for h, w in sizes])
    dst = torch.empty(total, device=dev, dtype=torch.uint8)
    transform_flat(src, [where[id(t)] for t in images], dst, dst_offsets, sizes, ops)
    return [dst[off:off + 3 * h * w].view(*out_size(h, w, op), 3) for off, (h, w), op in zip(dst_offsets, sizes, ops)]


def self_ensemble_on_device(groups, return_mean01=False):
    """``groups`` = ``[[(uint8 tensor, op), ...], ...]``: per merged image its 1 .. 8 sources on the GPU, source j being
    ``apply(x_j, op_j)`` of an ``[H,W,3]`` image (so ``[H,W,3]`` for op < 4, ``[W,H,3]`` for op >= 4) -> the list of merged uint8
    ``[H,W,3]`` device tensors, (2 S + n) // (2 n) per byte of the sources turned back; every group in ONE batched call.  With
    ``return_mean01`` a list of ``(merged, mean01 [1,3,H,W] fp32)``.  ``ValueError``: shapes, dtypes, ops or source sizes that do not
    fit each other; CPU tensors: ``SrgdHipError``."""
    if not isinstance(groups, (list, tuple)) or not groups:
        raise ValueError("self_ensemble_on_device: a non-empty list of source lists")
    sizes = []
    for g in groups:
        if not isinstance(g, (list, tuple)) or not 1 <= len(g) <= MAX_SOURCES or any(not isinstance(s, (list, tuple)) or len(s) != 2 for s in g):
            raise ValueError(f"self_ensemble_on_device: every image has 1 .. {MAX_SOURCES} (tensor, op) sources")
        _check_images("self_ensemble_on_device", [t for t, _ in g])
        turned = {out_size(int(t.shape[0]), int(t.shape[1]), inverse(op)) for t, op in g}
        if len(turned) != 1:
            raise ValueError("self_ensemble_on_device: the sources of an image, turned back, have different sizes")
        sizes.append(turned.pop())
    tensors = [t for g in groups for t, _ in g]
    dev = _one_gpu("the self-ensemble merge", tensors)
    src, flat_offs = gather(tensors, dev)
    src_offsets, at = [], 0
    for g in groups:
        src_offsets.append(flat_offs[at:at + len(g)])
        at += len(g)
    dst_offsets, total = layout([3 * h * w for h, w in sizes])
    m_offsets, m_total = [], 0
    for h, w in sizes:
        m_offsets.append(m_total)
        m_total += 3 * h * w
    dst = torch.empty(total, device=dev, dtype=torch.uint8)
    m01 = torch.empty(m_total, device=dev, dtype=torch.float32) if return_mean01 else None
    merge_flat(src, src_offsets, [[op for _, op in g] for g in groups], dst, dst_offsets, sizes, m01, m_offsets if return_mean01 else None)
    merged = [dst[off:off + 3 * h * w].view(h, w, 3) for off, (h, w) in zip(dst_offsets, sizes)]
    if not return_mean01:
        return merged
    return [(m, m01[off:off + 3 * h * w].view(1, 3, h, w)) for m, off, (h, w) in zip(merged, m_offsets, sizes)]
