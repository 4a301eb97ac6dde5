"""Yardsticks and inputs of the region-resampling tests (tests/test_region_cpu.py, tests/test_region_gpu.py).

(a) ``brute_active``: the tiles a region run evaluates, restated by painting - R as a boolean canvas, a tile is active where it
    covers a painted pixel.  Shares nothing with ``srgd_amd.region.active_tiles`` but the tile lists.
(b) ``region_tiled_sample``: the tiled loop of ``tests.guidance_cases.guided_tiled_sample`` (the oracle's own functions) plus the
    replacement step after every step, with the known image's noise z_i from ``oracle/philox.py`` (stream ``(3 << 32) | i``; the
    start canvas takes index ``num_sample_steps``) and the sampler's own draws from the caller's noise source.  It evaluates every
    tile of every step: skipping is the engine's business, and the comparison checks it too.
The cases and the oracle run are made once per session and shared, read-only."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import philox as PH
from oracle import srgd_oracle as O
from srgd_amd.lockstep import image_plan
from tests import guidance_cases as G

# planning: condition sizes (H, W) - one tile; 9 / 4 tiles with pulled-back last tiles; a non-square canvas; 25 / 16 tiles
GEOMETRIES = [(256, 256), (300, 300), (480, 320), (1024, 1024)]
# the tile-count case: on the 1024^2 image (crop box at 128, even seams at canvas 256 k, odd seams at 128 + 256 k) the box covers
# canvas [480, 672) on both axes - across the even seam at 512 and the odd seam at 640: 4 of 25 and 4 of 16 tiles
COUNT_CASE = dict(size=(1024, 1024), boxes=[(352, 352, 192, 192)], counts=([4], [4]), grids=(25, 16))
# the exactness case: a 64 x 64 box across the even seam at canvas 512 (image 384) on both axes
EXACT_CASE = dict(size=(1024, 1024), boxes=[(352, 352, 64, 64)])


def boxes_of(h, w):
    """Box lists of an ``h x w`` image: the corners, across the tile seams, one pixel, the whole image, an overlapping pair."""
    cy, cx = h // 2, w // 2
    lists = [[(0, 0, 1, 1)], [(h - 1, w - 1, 1, 1)], [(0, w - 7, 5, 7)], [(h - 3, 0, 3, 9)], [(0, 0, h, w)],
             [(cy, cx, 1, 1)], [(max(0, cy - 20), max(0, cx - 20), min(40, h), min(40, w))],
             [(0, 0, min(h, 30), min(w, 30)), (min(h - 1, 20), min(w - 1, 20), 1, 1), (h - 1, 0, 1, w)]]
    if h > 256:                                                     # across every seam of both grids: canvas rows 256 k and 128 + 256 k
        p = image_plan(h, w)
        top, left = p.box[1], p.box[0]
        for seam in (256, 384, 512):
            if top < seam < top + h - 1 and left < seam < left + w - 1:
                lists.append([(seam - top - 1, seam - left - 1, 2, 2)])
                lists.append([(seam - top, seam - left, 1, 1)])
    return lists


def brute_active(coords, hp, wp, top, left, boxes):
    """Indices of the tiles of ``coords`` that cover a pixel of R, by painting R on a boolean canvas."""
    canvas = np.zeros((hp, wp), dtype=bool)
    for (t, l, h, w) in boxes:
        canvas[top + t:top + t + h, left + l:left + l + w] = True
    return [j for j, (hs, he, ws, we) in enumerate(coords) if canvas[hs:he, ws:we].any()]


def brute_runs(indices):
    """Maximal runs of consecutive indices, by walking a boolean line."""
    if not indices:
        return []
    line = np.zeros(max(indices) + 2, dtype=bool)
    line[list(indices)] = True
    runs, j = [], 0
    while j < len(line):
        if line[j]:
            k = j
            while line[k]:
                k += 1
            runs.append((j, k - j))
            j = k
        else:
            j += 1
    return runs


# ------------------------------------------------------------------------------------------- (b) the region oracle
def region_noise(index, seed, hp, wp):
    """z of the draw named ``index``: what ``srgd_randn(seed, (3 << 32) | index)`` writes on a [3,Hp,Wp] canvas, float64 restatement
    rounded to float32."""
    z = PH.philox_normal(3 * hp * wp, seed, (3 << 32) | index)
    return torch.from_numpy(z.astype(np.float32)).reshape(1, 3, hp, wp)


def region_tiled_sample(sd, cfg, condition_x, class_label, known01, boxes, seed, *, batch_size=4, num_sample_steps=4,
                        class_cond_scale=1.0, tile=256, noise=None, trace=None):
    """``guided_tiled_sample`` without the guidance and with the replacement step: after the start canvas and after every step the
    canvas outside R is alpha k + sigma z_i on the reflect-padded known image k = 2 known - 1, ``x_start`` outside R is k."""
    noise = noise or O.NoiseSource()
    cond = condition_x * 2 - 1
    _, _, h, w = cond.shape
    (left, top, right, bottom), pad = O.canvas_box_and_pad(h, w)
    cond = F.pad(cond, pad, mode="reflect")
    k_pad = F.pad(known01 * 2 - 1, pad, mode="reflect")
    hp, wp = cond.shape[-2:]
    inside = torch.zeros(1, 1, hp, wp, dtype=torch.bool)
    for (t, l, bh, bw) in boxes:
        inside[:, :, top + t:top + t + bh, left + l:left + l + bw] = True

    def replaced(canvas, alpha, sigma, index):
        known = k_pad * alpha + region_noise(index, seed, hp, wp) * sigma if index is not None else k_pad
        return torch.where(inside, canvas, known)

    ls0 = O.log_snr_linear(torch.tensor(1.0))
    img = replaced(noise.randn(cond.shape), ls0.sigmoid().sqrt(), (-ls0).sigmoid().sqrt(), num_sample_steps)
    steps = torch.linspace(1.0, 0.0, num_sample_steps + 1)
    grids = O.sampling_grids(hp, wp, tile, tile)
    (il, it, ir, ib), ipad = O.grid_bbox(grids[1], hp, wp)
    cond = F.pad(cond[:, :, it:ib, il:ir], ipad, mode="constant", value=0.0)
    x_start = img.clone()
    for i in range(num_sample_steps):
        ccs = class_cond_scale
        t, t_next = steps[i], steps[i + 1]
        grid = grids[i % 2]
        for j in range(0, len(grid), batch_size):
            chunk = grid[j:j + batch_size]
            xb = torch.cat([img[:, :, a:b, c:d] for (a, b, c, d) in chunk], dim=0)
            cb = torch.cat([cond[:, :, a:b, c:d] for (a, b, c, d) in chunk], dim=0)
            out, x0 = O.predict_and_step(sd, cfg, xb, t, t_next, cb, class_label, 1.0, ccs, noise, trace)
            for k, (a, b, c, d) in enumerate(chunk):
                img[:, :, a:b, c:d] = out[k]
                x_start[:, :, a:b, c:d] = x0[k]
        if i % 2 == 1:                                              # the sampler's own ring draw: replaced below, but drawn
            inner = img[:, :, it:ib, il:ir].clone()
            sigma = (-O.log_snr_linear(t_next)).sigmoid().sqrt()
            img = noise.randn(cond.shape) * sigma
            img[:, :, it:ib, il:ir] = inner
        if i == num_sample_steps - 1:
            img = replaced(img, None, None, None)
        else:
            ls_next = O.log_snr_linear(t_next)
            img = replaced(img, ls_next.sigmoid().sqrt(), (-ls_next).sigmoid().sqrt(), i)
        x_start = replaced(x_start, None, None, None)
        if trace is not None:
            trace.setdefault("img", []).append(img.clone())
            trace.setdefault("x_start", []).append(x_start.clone())
    out = (img[:, :, top:bottom, left:right].clamp(-1.0, 1.0) + 1) * 0.5
    outside = ~inside[:, :, top:bottom, left:right]
    return torch.where(outside, known01, out)


# the end-to-end case: the 300 x 300 geometry (9 / 4 tiles), 4 steps under class guidance 2.0; two boxes, one across the even seam
# at canvas 256 and one pixel wide at the far corner
ORACLE_CASE = dict(lr=(75, 75), steps=4, class_cond_scale=2.0, batch_size=4, seed=71, lr_seed=2, known_seed=5,
                   boxes=[(10, 20, 60, 50), (299, 299, 1, 1)])


@functools.lru_cache(maxsize=None)
def oracle_input():
    """(condition [1,3,300,300], known image [1,3,300,300]) of the end-to-end case, float32 in [0, 1]."""
    case = ORACLE_CASE
    cond = G.condition_of(G.smooth_lr(*case["lr"], case["lr_seed"]))
    known = G.condition_of(G.smooth_lr(*case["lr"], case["known_seed"]))
    return cond, known


@functools.lru_cache(maxsize=None)
def oracle_run():
    """(output [1,3,H,W], trace {"img": [...], "x_start": [...]}) of the region oracle on the end-to-end case.  Host noise after
    ``torch.manual_seed(seed)``; the caller's generator is restored."""
    case = ORACLE_CASE
    cond, known = oracle_input()
    state = torch.get_rng_state()
    torch.manual_seed(case["seed"])
    trace = {}
    with torch.inference_mode():
        out = region_tiled_sample(O.strip_model_prefix(G.state_dict()), O.UnetCfg(dim=G.DIM), cond, torch.tensor([G.LABEL]), known,
                                  case["boxes"], case["seed"], batch_size=case["batch_size"], num_sample_steps=case["steps"],
                                  class_cond_scale=case["class_cond_scale"], trace=trace)
    torch.set_rng_state(state)
    return out, {k: v for k, v in trace.items() if k in ("img", "x_start")}
