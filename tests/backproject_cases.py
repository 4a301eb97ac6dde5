"""Yardstick and inputs of the back-projection tests (tests/test_backproject_cpu.py, tests/test_backproject_gpu.py).

The yardstick is Pillow itself (include/srgd_backproject.h): one step is ``O <- clip(O + C - pillow_up(pillow_down(O)), 0, 255)`` with
the two ``Image.resize(BICUBIC)`` calls of tests/consistency_cases.py and int64 numpy between them.  Everything is an exact integer, so
every comparison with the GPU is an equality.  ``quant_out`` (q) and ``quant_cond`` (r) restate the header's two quantisations in
numpy float32.
Inputs: the LR sizes of tests/consistency_cases.py and the three kinds of tests/test_consistency_gpu.py - seeded random bytes, the
overshoot image (0 / 255 blocks), and ``O`` = Pillow x4 of ``L`` - with ``C`` = Pillow x4 of ``L``, the condition the sampler is given."""
import numpy as np

from tests import consistency_cases as K

SIZES = K.SIZES
KINDS = ("random", "overshoot", "up")
F255 = np.float32(255.0)
_cache = {}


def quant_out(v):
    """q: t = v * 255 in float32; 0 where t is NaN or <= 0, 255 where t >= 255, truncation otherwise -> uint8."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(v, dtype=np.float32) * F255
        low = np.isnan(t) | (t <= 0)
        high = ~low & (t >= F255)
        mid = np.trunc(np.where(low | high, np.float32(0), t))
    return np.where(low, 0, np.where(high, 255, mid)).astype(np.uint8)


def quant_cond(v):
    """r: 0 for NaN, otherwise clamp(floor(v * 255 + 0.5), 0, 255), every operation rounded to float32 -> uint8."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor(np.asarray(v, dtype=np.float32) * F255 + np.float32(0.5))
        t = np.where(np.isnan(t), np.float32(0), t)
    return np.clip(t, 0, 255).astype(np.uint8)


def unit(img_u8):
    """uint8 [H,W,3] -> float32 planar [3,H,W] = u8 / 255: ToTensor of the saved file, the library's result format."""
    return np.ascontiguousarray((img_u8.astype(np.float32) / F255).transpose(2, 0, 1))


def raw_step(out, cond):
    """O + C - U before the clip, int64 [H,W,3]."""
    up = K.pillow_up(K.pillow_down(out))
    return out.astype(np.int64) + cond.astype(np.int64) - up.astype(np.int64)


def step(out, cond):
    """One back-projection step on uint8 [H,W,3] images."""
    return np.clip(raw_step(out, cond), 0, 255).astype(np.uint8)


def steps(out, cond, n):
    """[O_0, O_1, ..., O_n]."""
    seq = [out]
    for _ in range(n):
        seq.append(step(seq[-1], cond))
    return seq


def case(kind, h, w):
    """(O_0 uint8 [4h,4w,3], C uint8 [4h,4w,3], L uint8 [h,w,3], [O_0 .. O_5] of the yardstick): computed once per session, shared,
    read-only.  The pairs (O_0, L) are those of tests/test_consistency_gpu.py."""
    key = (kind, h, w)
    if key not in _cache:
        if kind == "random":
            out, lr = K.random_pair(h, w, 7)
        elif kind == "overshoot":
            out, lr = K.overshoot_output(h, w), K.random_pair(h, w, 8)[1]
        else:                                                    # "up": O = Pillow x4 of L
            lr = K.random_pair(h, w, 9)[1]
            out = K.pillow_up(lr)
        out, lr = np.ascontiguousarray(out), np.ascontiguousarray(lr)
        cond = np.ascontiguousarray(K.pillow_up(lr))
        seq = steps(out, cond, 5)
        for a in [out, lr, cond] + seq:
            a.setflags(write=False)
        _cache[key] = (out, cond, lr, seq)
    return _cache[key]
