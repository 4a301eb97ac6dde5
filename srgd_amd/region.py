"""Region resampling: a finished output is kept and rectangles of it are drawn again (``tiled_sample(region_known=...,
regions=...)``, ``--region_known_dir`` / ``--region``), RePaint-style - after every step the canvas outside the union R of the
rectangles is replaced by the known image forward-diffused to the step's end level, so that what is sampled inside R grows
coherent with its surroundings - and only the tiles that touch R are evaluated.

Everything here is host-side planning (pure ints) and the driver of existing device work: the engine's ``srgd_sampler_q_start``
(the known image onto a whole padded canvas at a level, reflect padding included), ``srgd_randn`` (the named Philox stream of the
draw) and strided device copies.  No arithmetic happens in this file.

Noise of the known image's forward diffusion: the draw after loop index i comes from ``srgd_randn`` with the image's noise seed
and stream id ``(3 << 32) | i`` (high words 0, 1 and 2 are the sampler's own streams); the draw of the start
canvas, which belongs to no loop index, uses index ``num_sample_steps`` - the last loop index draws nothing, so it is free.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

MAX_BOXES = 16
STREAM_HIGH = 3
TILE = 256

Box = Tuple[int, int, int, int]           # (top, left, height, width) in output pixels


def region_stream_id(index: int) -> int:
    """The Philox stream of the known image's noise after loop index ``index`` (``num_sample_steps``: the start canvas)."""
    return (STREAM_HIGH << 32) | (int(index) & 0xFFFFFFFF)


# --------------------------------------------------------------------------------------------- checks
def check_boxes(boxes, height: int, width: int) -> Tuple[Box, ...]:
    """``regions`` of one ``height x width`` image as a tuple of int boxes: 1 .. 16 of them, each ``(top, left, height, width)``
    with a positive size and inside the image (they may overlap).  ``ValueError`` otherwise."""
    import operator
    try:
        boxes = list(boxes)
    except TypeError:
        raise ValueError("regions: a list of (top, left, height, width) boxes")
    if not 1 <= len(boxes) <= MAX_BOXES:
        raise ValueError(f"regions: 1 .. {MAX_BOXES} boxes per image, got {len(boxes)}")
    out = []
    for b in boxes:
        try:
            t, l, h, w = (operator.index(v) for v in b)
        except (TypeError, ValueError):
            raise ValueError(f"regions: {b!r} is not a (top, left, height, width) box of integers")
        if h < 1 or w < 1 or t < 0 or l < 0 or t + h > height or l + w > width:
            raise ValueError(f"regions: box (top {t}, left {l}, height {h}, width {w}) is empty or outside the {height}x{width} image")
        out.append((t, l, h, w))
    return tuple(out)


def _is_flat_box_list(regions) -> bool:
    try:
        first = regions[0]
        return not isinstance(first[0], (list, tuple))
    except (TypeError, IndexError, KeyError):
        return False


def check_region_args(region_known, regions, sizes: Sequence[Tuple[int, int]]):
    """``tiled_sample(region_known=..., regions=...)`` for a run on images of ``sizes`` [(H, W)]: None without both keywords, else
    one entry per image, ``None`` (sampled whole) or ``(known fp32 [1,3,H,W], boxes)``.

    ``region_known``: one fp32 ``[1,3,H,W]`` tensor (a run on one image), a ``[B,3,H,W]`` tensor, or a list with one entry per
    image whose ``None`` entries are the images sampled whole.  ``regions``: one list of boxes for every image that has a known
    image, or - in a group - a list with one list of boxes (or ``None``) per image.  ``ValueError``: one keyword without the
    other, a known image of another shape or dtype than its condition, a group without any known image, bad boxes."""
    if region_known is None and regions is None:
        return None
    if region_known is None:
        raise ValueError("regions without region_known (the finished image the regions are drawn into)")
    if regions is None:
        raise ValueError("region_known without regions (the boxes to sample again)")
    n = len(sizes)
    if torch.is_tensor(region_known):
        if region_known.dim() != 4 or region_known.shape[0] != n:
            raise ValueError(f"region_known: a [{n},3,H,W] tensor for {n} image(s), got {tuple(region_known.shape)}")
        known = [region_known[i:i + 1] for i in range(n)]
    elif isinstance(region_known, (list, tuple)):
        if len(region_known) != n:
            raise ValueError(f"region_known: {len(region_known)} entries for {n} images (one per image, None: sampled whole)")
        known = list(region_known)
    else:
        raise ValueError("region_known: a fp32 [1,3,H,W] tensor, or a list of one (or None) per image")
    if not any(k is not None for k in known):
        raise ValueError("region_known: no image of the group has a known image")
    try:
        regions = list(regions)
    except TypeError:
        raise ValueError("regions: a list of (top, left, height, width) boxes")
    if _is_flat_box_list(regions) or not regions:
        per_image = [regions if k is not None else None for k in known]
    else:
        if len(regions) != n:
            raise ValueError(f"regions: {len(regions)} box lists for {n} images (one per image)")
        per_image = regions
    out = []
    for i, ((h, w), k, boxes) in enumerate(zip(sizes, known, per_image)):
        if k is None:
            if boxes is not None:
                raise ValueError(f"regions: image {i} has boxes and no region_known")
            out.append(None)
            continue
        if boxes is None:
            raise ValueError(f"region_known: image {i} has a known image and no boxes")
        if not torch.is_tensor(k) or k.dtype != torch.float32 or tuple(k.shape) != (1, 3, h, w):
            got = (tuple(k.shape), k.dtype) if torch.is_tensor(k) else type(k).__name__
            raise ValueError(f"region_known: image {i} must be fp32 [1,3,{h},{w}] like its condition_x, got {got}")
        out.append((k, check_boxes(boxes, h, w)))
    return out


# --------------------------------------------------------------------------------------------- planning (pure ints)
def active_tiles(coords, top: int, left: int, boxes: Sequence[Box]) -> List[int]:
    """Indices into ``coords`` (a grid's tile boxes ``(hs, he, ws, we)`` in canvas coordinates) of the tiles that share at least
    one pixel with a box of ``boxes`` (image coordinates; the image sits at ``(top, left)`` of its canvas), ascending."""
    out = []
    for j, (hs, he, ws, we) in enumerate(coords):
        for (t, l, h, w) in boxes:
            if hs < top + t + h and top + t < he and ws < left + l + w and left + l < we:
                out.append(j)
                break
    return out


def tile_runs(indices: Sequence[int]) -> List[Tuple[int, int]]:
    """Ascending tile indices as maximal runs of consecutive ones: ``[(first, count)]``."""
    runs: List[List[int]] = []
    for j in indices:
        if runs and runs[-1][0] + runs[-1][1] == j:
            runs[-1][1] += 1
        else:
            runs.append([j, 1])
    return [(a, b) for a, b in runs]


def plan_region_steps(images, skip_tiles: bool = True):
    """The tiles a region run evaluates.  ``images``: per image ``(coords0, coords1, top, left, boxes or None)`` in the order of
    the engine's image-major tile lists.  Returns ``(runs, counts)``, each indexed by step parity: ``runs[p]`` the
    ``srgd_sampler_step_tiles`` calls ``[(first, count)]`` of a step on grid p, ``counts[p]`` the evaluated tiles per image.  An
    image without boxes, and every image when ``skip_tiles`` is off, takes all its tiles."""
    runs, counts = [], []
    for p in (0, 1):
        base, wanted, per_image = 0, [], []
        for im in images:
            coords, boxes = im[p], im[4]
            local = list(range(len(coords))) if (boxes is None or not skip_tiles) else active_tiles(coords, im[2], im[3], boxes)
            wanted.extend(base + j for j in local)
            per_image.append(len(local))
            base += len(coords)
        runs.append(tile_runs(wanted))
        counts.append(per_image)
    return runs, counts


# --------------------------------------------------------------------------------------------- the run
class RegionImage:
    """One image of a region run: where its canvas and its output lie in the run's flat buffers, its geometry, its boxes."""

    def __init__(self, canvas_off, out_off, hp, wp, top, left, h, w, coords0, coords1, noise_class, boxes):
        self.canvas_off, self.out_off = int(canvas_off), int(out_off)
        self.hp, self.wp, self.top, self.left, self.h, self.w = hp, wp, top, left, h, w
        self.coords = (coords0, coords1)
        self.noise_class = noise_class
        self.boxes = boxes


class _RegionRun:
    """The region resampling of one DDPM run, next to ``_GuidedRun`` / ``_ThresholdRun`` / ``_SolverRun`` in the drivers: the tile
    ranges of both step parities are planned once, ``replace`` is the replacement step on the run's canvases, ``composite`` the
    final copy on its outputs.

    Buffers (made once): the known images laid out like ``cond01``, the noise of one draw laid out per noise class as
    ``srgd_sampler_q_start`` reads host noise, the scratch canvas K, and K at (1, 0) - the padded known image itself, which the
    ``x_start`` canvas and the last step take."""

    def __init__(self, eng, images: Sequence[RegionImage], known, classes, class_seeds, num_sample_steps, skip_tiles, dev,
                 total_canvas, total_out):
        self.eng, self.images, self.dev = eng, list(images), dev
        self.classes, self.class_seeds = list(classes), [int(s) for s in class_seeds]
        self.num_sample_steps = num_sample_steps
        self.runs, self.counts = plan_region_steps([(m.coords[0], m.coords[1], m.top, m.left, m.boxes) for m in self.images], skip_tiles)
        self.log: List[List[int]] = []
        self.known01 = torch.zeros(total_out, device=dev, dtype=torch.float32)
        for m, k in zip(self.images, known):
            if k is not None:
                self.known01[m.out_off:m.out_off + 3 * m.h * m.w].copy_(k.to(dev, torch.float32).reshape(-1))
        self.class_offs = [0]
        for (hp, wp) in self.classes:
            self.class_offs.append(self.class_offs[-1] + 3 * hp * wp)
        self.noise = torch.zeros(self.class_offs[-1], device=dev, dtype=torch.float32)
        self.k_level = torch.empty(total_canvas, device=dev, dtype=torch.float32)
        self.k_clean = torch.empty(total_canvas, device=dev, dtype=torch.float32)
        eng.sampler_q_start(self.known01, self.noise, 1.0, 0.0, self.k_clean)           # 1 * k + 0 * 0: the padded known image

    # ---- steps
    def step_ranges(self, i):
        """The ``(first, count, do_ring)`` calls of step i; its per-image counts go to the log.  The ring re-noise of an odd step
        lies outside R and is replaced after the step, so it is skipped - unless the group holds an image that is sampled whole,
        whose ring the last call of the step then draws as that image's own run does."""
        self.log.append(list(self.counts[i % 2]))
        runs = self.runs[i % 2]
        ring = any(m.boxes is None for m in self.images)
        return [(first, count, ring and j == len(runs) - 1) for j, (first, count) in enumerate(runs)]

    def _view(self, flat, m):
        return flat.view(-1)[m.canvas_off:m.canvas_off + 3 * m.hp * m.wp].view(3, m.hp, m.wp)

    def _keep_boxes(self, canvas, k):
        """canvas := k outside R, canvas inside R - for every image with boxes: R of ``canvas`` into ``k``, ``k`` over ``canvas``."""
        for m in self.images:
            if m.boxes is None:
                continue
            cv, kv = self._view(canvas, m), self._view(k, m)
            for (t, l, h, w) in m.boxes:
                kv[:, m.top + t:m.top + t + h, m.left + l:m.left + l + w].copy_(cv[:, m.top + t:m.top + t + h, m.left + l:m.left + l + w])
            cv.copy_(kv)

    def replace(self, index, alpha, sigma, img, x_start=None):
        """The replacement step at ``(alpha, sigma)``: ``index`` names the draw (a loop index, or ``num_sample_steps`` for the
        start canvas); ``None``: the level (1, 0), no draw."""
        if index is None:
            self._keep_boxes(img, self.k_clean)
        else:
            for k, seed in enumerate(self.class_seeds):
                self.eng.randn_(self.noise[self.class_offs[k]:self.class_offs[k + 1]], seed, region_stream_id(index))
            self.eng.sampler_q_start(self.known01, self.noise, float(alpha), float(sigma), self.k_level)
            self._keep_boxes(img, self.k_level)
        if x_start is not None:
            self._keep_boxes(x_start, self.k_clean)

    def after_step(self, i, scalars, img, x_start=None):
        """The replacement step after loop index i: at the step's end level; the last step ends at (1, 0)."""
        if i == self.num_sample_steps - 1:
            self.replace(None, 1.0, 0.0, img, x_start)
        else:
            self.replace(i, scalars[i].alpha_next, scalars[i].sigma_next, img, x_start)

    # ---- the end
    def composite(self, out):
        """``out`` (flat, laid out like ``cond01``) outside R := the known image, by copy."""
        for m in self.images:
            if m.boxes is None:
                continue
            ov = out.view(-1)[m.out_off:m.out_off + 3 * m.h * m.w].view(3, m.h, m.w)
            kv = self.known01[m.out_off:m.out_off + 3 * m.h * m.w].view(3, m.h, m.w)
            for (t, l, h, w) in m.boxes:
                kv[:, t:t + h, l:l + w].copy_(ov[:, t:t + h, l:l + w])
            ov.copy_(kv)
