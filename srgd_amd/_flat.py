"""Flat uint8 device buffers for the batched byte kernels (resize, alpha, selfens): images lie at 16-byte aligned offsets of one
buffer.  The layout, the packing of a list of tensors, the argument checks and the look for a device, once.  Torch allocates and
copies here; nothing is computed."""
from __future__ import annotations

import torch

from . import _lib

ALIGN = 16                                                # offsets, and every image's part of a scratch, are multiples of it


def round16(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def layout(nbytes):
    """``[bytes of image i]`` -> (offsets, total): the images one after the other, each at a multiple of 16."""
    offsets, total = [], 0
    for n in nbytes:
        offsets.append(total)
        total += round16(n)
    return offsets, total


def device_of(tensors, what):
    """The device of the first GPU tensor, else the current GPU; ``SrgdHipError`` where there is none."""
    dev = next((t.device for t in tensors if t.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise _lib.SrgdHipError(f"{what} runs on MI355X only (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def gather(tensors, dev):
    """The tensors, flattened, at 16-byte aligned offsets of one flat uint8 device buffer -> (buffer, offsets)."""
    offsets, total = layout([t.numel() for t in tensors])
    buf = torch.empty(max(total, ALIGN), device=dev, dtype=torch.uint8)
    for t, off in zip(tensors, offsets):
        buf[off:off + t.numel()].copy_(t.reshape(-1), non_blocking=True)
    return buf, offsets


def check_buffers(what, buffers, subject=None):
    """Contiguous flat uint8 device buffers on one device.  ``subject``: ``what`` as the subject of a sentence, where it differs."""
    if not all(t.is_cuda for t in buffers):
        raise _lib.SrgdHipError(f"{subject or what} runs on MI355X only (no CPU fallback)")
    for t in buffers:
        if t.dtype != torch.uint8 or not t.is_contiguous() or t.device != buffers[0].device or t.dim() != 1:
            raise ValueError(f"{what}: flat contiguous uint8 buffers on one device")


def check_spans(what, n, *spans):
    """``spans``: (buffer, offsets, [bytes of image i]) - n >= 1 images, one offset per image, multiples of 16, every image inside
    its buffer."""
    for buf, offsets, sizes in spans:
        if n < 1 or len(offsets) != len(sizes) or min(offsets) < 0 or any(off % ALIGN for off in offsets) \
                or max(off + size for off, size in zip(offsets, sizes)) > buf.numel():
            raise ValueError(f"{what}: offsets / sizes do not fit the buffers")


def check_flat(what, buffers, n, *spans):
    """``check_buffers``, then ``check_spans``."""
    check_buffers(what, buffers)
    check_spans(what, n, *spans)
