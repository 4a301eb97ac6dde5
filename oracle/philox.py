"""CPU restatement of the engine's device-noise generator (TEST INFRASTRUCTURE ONLY, like the rest of ``oracle/``).

``philox_normal_kernel`` (srgd_amd/csrc/sampler.hip) is a pure function of ``(seed, stream_id, step, element index)``:
Philox4x32-10 on the counter ``(q lo, q hi, stream_id lo, stream_id hi ^ (step << 8))`` with the key ``(seed lo, seed hi)``,
then two Box-Muller pairs per quad ``q``.  This module restates it in numpy so that a test can hand the CPU oracle exactly the
noise a device-noise run draws (``device_noise_draws`` -> ``srgd_oracle.ReplayNoise``).

What is restated bit for bit: the integer generator and the float32 roundings of ``u1``, ``u2`` and ``theta``.  What is not:
the device's ``__logf`` / ``sqrtf`` / ``__sincosf`` and the two float32 products - the default output evaluates those in
float64 on the float32 arguments; ``dtype=np.float32`` evaluates them with numpy's float32 functions and exists only to
measure how far float32 arithmetic of any make sits from the float64 value (the rounding floor of the device comparison).

Step limit: the step is mixed in as ``(uint32)step << 8`` - steps ``0 .. 2^24 - 1`` are distinct, step ``2^24`` wraps onto
step 0; and the low byte of the high stream word is left to the stream ids, which use bits 32..33 only.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57      # multipliers of c[0] and c[2]
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85      # Weyl increments of the key
TWO_PI_F32 = np.float32(6.283185307179586)         # the kernel's literal 6.283185307179586f
INV_2_32 = np.float32(2.3283064365386963e-10)      # 2^-32

# stream ids of the engine (srgd_amd/csrc/engine.hip, srgd_amd/model.py)
STREAM_START = 0                                   # DDPM start canvas and q_sample start; un-tiled start
STREAM_EDM_START = 1                               # EDM start canvas / noised start
STREAM_TILES = 1 << 32                             # DDPM per-step tile noise (step mixed in)
STREAM_RING = (1 << 32) | 0x80000000               # odd-step ring re-noise canvas, DDPM and EDM (step mixed in)
STREAM_EDM_EPS = 2 << 32                           # EDM per-step eps canvas (step mixed in)


def counter_words(stream_id: int, step: Optional[int]):
    """The two counter words that do not depend on the element: (c[2], c[3])."""
    s = 0 if step is None else int(step)
    return int(stream_id) & M32, ((int(stream_id) >> 32) & M32) ^ ((s << 8) & M32)


def philox4x32_10(counter, key) -> np.ndarray:
    """counter: four uint32 words (scalars or arrays that broadcast), key: two.  Returns uint32 [..., 4]."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & np.uint64(M32) for v in counter])
    k0, k1 = (int(key[0]) & M32, int(key[1]) & M32)
    m32 = np.uint64(M32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0                  # < 2^64: both factors < 2^32
        p1 = np.uint64(PHILOX_M1) * c2
        n0 = (p1 >> s32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> s32) ^ c3 ^ np.uint64(k1)
        c1, c3 = p1 & m32, p0 & m32
        c0, c2 = n0, n2
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def box_muller(c: np.ndarray, dtype=np.float64) -> np.ndarray:
    """The kernel's tail: uint32 [nq, 4] generator words -> [nq, 4] normals (r0 cos t0, r0 sin t0, r1 cos t1, r1 sin t1) with
    ``r_h = sqrt(-2 ln u1_h)``, ``u1_h = fl32((fl32(c[2h]) + 1) * 2^-32)`` in (0, 1] and
    ``t_h = fl32(6.2831855f * fl32(fl32(c[2h+1]) * 2^-32))``.  ``u1 = 1`` (words >= 2^32 - 128) gives r = 0, not a NaN."""
    c = np.asarray(c, dtype=np.uint32)
    one = np.float32(1.0)
    z = np.empty(c.shape, dtype=dtype)
    for h in range(2):
        u1 = (c[:, 2 * h].astype(np.float32) + one) * INV_2_32
        u2 = c[:, 2 * h + 1].astype(np.float32) * INV_2_32
        theta = TWO_PI_F32 * u2
        assert u1.dtype == np.float32 and theta.dtype == np.float32
        if dtype == np.float32:
            rad = np.sqrt(np.float32(-2.0) * np.log(u1))
            cs, sn = np.cos(theta), np.sin(theta)
        else:
            rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
            cs, sn = np.cos(theta.astype(np.float64)), np.sin(theta.astype(np.float64))
        z[:, 2 * h] = rad * cs
        z[:, 2 * h + 1] = rad * sn
    return z


def philox_words(n: int, seed: int, stream_id: int, step: Optional[int] = None) -> np.ndarray:
    """The generator words behind the first n normals of a stream: uint32 [ceil(n/4), 4]."""
    seed = int(seed) & (2 ** 64 - 1)
    q = np.arange((int(n) + 3) // 4, dtype=np.uint64)
    w2, w3 = counter_words(stream_id, step)
    return philox4x32_10((q & np.uint64(M32), q >> np.uint64(32), w2, w3), (seed & M32, seed >> 32))


def philox_normal(n: int, seed: int, stream_id: int, step: Optional[int] = None, dtype=np.float64) -> np.ndarray:
    """What ``philox_normal_kernel(dst, n, seed, stream_id, step_ptr)`` writes; ``step=None`` is the null ``step_ptr``.

    Quad q (counter ``(q lo, q hi, stream_id lo, stream_id hi ^ (step << 8))``, key ``(seed lo, seed hi)``) gives
    ``z[4q .. 4q+3]`` (``box_muller``); the last quad is cut at n.  float64 output: log / sqrt / cos / sin and the products in
    float64 on the float32 arguments; ``dtype=np.float32``: numpy's float32 functions (the rounding-floor twin)."""
    return box_muller(philox_words(n, seed, stream_id, step), dtype).reshape(-1)[:int(n)]


# --------------------------------------------------------------------------------------
# the draws of a device-noise run, in the oracle's order
# --------------------------------------------------------------------------------------
def _t(z: np.ndarray, *shape):
    import torch
    return torch.from_numpy(z.astype(np.float32)).reshape(*shape)


def device_noise_draws(kind: str, *, seed: int, num_sample_steps: int, generation_start_steps: int = 0,
                       height: Optional[int] = None, width: Optional[int] = None, batch_size: int = 4,
                       batch: Optional[int] = None, image_size: int = 256, tile: int = 256, zero_init: bool = False,
                       tile_step_of=None) -> List["torch.Tensor"]:
    """The tensors the oracle's sampler asks its noise source for, in its order, each cut out of the buffer the ENGINE draws
    in device-noise mode (float64 restatement rounded to float32) - for ``srgd_oracle.ReplayNoise``.

    Step value: the engine writes the LOOP INDEX ``i`` to its device-side step counter (``set_step_kernel`` launched by
    ``srgd_sampler_step_tiles`` / ``srgd_edm_step_tiles`` with their ``step`` argument, which model.py passes as ``i``) - not a
    count of executed steps: after a skipped ``generation_start_steps`` prefix the first executed step mixes in
    ``generation_start_steps``.

    kind "ddpm_tiled" (``srgd_oracle.tiled_sample``; ``height`` x ``width`` image, oracle minibatch ``batch_size``):
      start canvas [1,3,Hp,Wp]: stream 0, no step - white-noise start and q_sample start alike;
      executed step i, not the last: ONE buffer of n_tiles(i % 2) * 3 * tile^2 normals, stream 1<<32, step i, viewed
      [n_tiles,3,tile,tile] (tile index inside the image, final_step_kernel's ``tl``), handed out in minibatch slices;
      odd i (the last included): the ring canvas [1,3,Hp,Wp], stream (1<<32)|0x80000000, step i.
    kind "edm_tiled" (``srgd_oracle.edm_tiled_sample``): start canvas stream 1, no step (none with ``zero_init``); executed
      step i: the eps canvas [1,3,Hp,Wp], stream 2<<32, step i (addressed per canvas pixel), then for odd i the ring canvas.
    kind "ddpm_sample" (``srgd_oracle.sample``; ``batch`` images of ``image_size``): the start is 3*b*S*S normals of stream 0
      in the canvas layout [3][b*S][S], read back as [b,3,S,S]; executed step i, not the last: [b,3,S,S], stream 1<<32, step i.

    ``tile_step_of``: maps the loop index to the step value of the per-step tile buffer (default: identity) - only for tests
    that replay a deliberately wrong plan."""
    from oracle import srgd_oracle as O
    n, g0 = int(num_sample_steps), int(generation_start_steps)
    tile_step_of = tile_step_of or (lambda i: i)
    draws = []
    if kind == "ddpm_sample":
        b, s = int(batch), int(image_size)
        start = philox_normal(3 * b * s * s, seed, STREAM_START)
        draws.append(_t(start, 3, b, s, s).permute(1, 0, 2, 3).contiguous())
        for i in range(g0, n - 1):
            draws.append(_t(philox_normal(b * 3 * s * s, seed, STREAM_TILES, tile_step_of(i)), b, 3, s, s))
        return draws
    _, pad = O.canvas_box_and_pad(height, width, tile)
    hp, wp = height + pad[2] + pad[3], width + pad[0] + pad[1]
    grids = O.sampling_grids(hp, wp, tile, tile)
    canvas = lambda stream, step=None: _t(philox_normal(3 * hp * wp, seed, stream, step), 1, 3, hp, wp)
    if kind == "ddpm_tiled":
        draws.append(canvas(STREAM_START))
        for i in range(g0, n):
            if i != n - 1:
                nt = len(grids[i % 2])
                buf = _t(philox_normal(nt * 3 * tile * tile, seed, STREAM_TILES, tile_step_of(i)), nt, 3, tile, tile)
                draws += [buf[j:j + batch_size] for j in range(0, nt, batch_size)]
            if i % 2 == 1:
                draws.append(canvas(STREAM_RING, i))
        return draws
    if kind == "edm_tiled":
        if g0 > 0 or not zero_init:
            draws.append(canvas(STREAM_EDM_START))
        for i in range(g0, n):
            draws.append(canvas(STREAM_EDM_EPS, i))
            if i % 2 == 1:
                draws.append(canvas(STREAM_RING, i))
        return draws
    raise ValueError(f"unknown kind {kind!r}")
