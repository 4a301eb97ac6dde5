"""Host-side planning of mixed-size lock-step (pure ints, no GPU): per-image geometry records, noise classes, and the CLI's
grouping of consecutive files under a tile budget.

A mixed group samples images of different sizes together: every image keeps its own canvas, crop box, reflect padding, inner
box and tile grids (reference model.py:3296-3342, exactly what a run of that image alone uses), and a step's tiles of all
images share the U-Net launches.  The reference reseeds before every image (inference.py:73) and its draw sequence depends
only on the canvas size, so images with the same canvas ``(Hp, Wp)`` form one *noise class* and share their noise, as
same-sized images in lock-step always have (480x320 and 320x480 both pad to 768x768: one class).  With per-image noise seeds
(``tiled_sample(seeds=...)``) a class is a noise stream, the pair (canvas size, seed): K copies of one image with K seeds
are K streams and come out as K different samples.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple


class ImagePlan(NamedTuple):
    H: int
    W: int
    Hp: int
    Wp: int
    box: Tuple[int, int, int, int]        # (left, top, right, bottom) of the image inside its canvas
    inner: Tuple[int, int, int, int]      # (left, top, right, bottom) bounding box of the odd grid
    coords0: list                         # even grid, [(hs, he, ws, we)]
    coords1: list                         # odd grid
    noise_class: int


def image_plan(h: int, w: int, tile_size: int = 256, noise_class: int = 0) -> ImagePlan:
    """Geometry of one ``h x w`` image as ``tiled_sample`` computes it for that image alone (raises on a reflect pad that
    F.pad refuses, as the reference does)."""
    from .model import _tiling
    box, (hp, wp), coords0, coords1, inner = _tiling(h, w, tile_size, tile_size)
    return ImagePlan(h, w, hp, wp, tuple(box), tuple(inner), coords0, coords1, noise_class)


def plan_mixed_group(sizes: Sequence[Tuple[int, int]], tile_size: int = 256, seeds: Optional[Sequence[int]] = None):
    """Per-image plans of a group and its noise classes: ``(plans, classes)`` with ``classes`` the canvas sizes ``(Hp, Wp)``
    in order of first appearance and ``plans[i].noise_class`` the index of image i's class.

    With ``seeds`` (one noise seed per image) a class is a *noise stream*, the pair (canvas size, seed): images that agree in
    both share one, images that differ in either get their own, numbered in order of first appearance.  The return value is
    then ``(plans, classes, class_seeds)``: ``classes[k]`` still the canvas size of stream k (sizes may repeat) and
    ``class_seeds[k]`` its seed."""
    if seeds is not None and len(seeds) != len(sizes):
        raise ValueError(f"seeds: {len(seeds)} seeds for {len(sizes)} images (one per image)")
    plans, classes, keys = [], [], []
    for i, (h, w) in enumerate(sizes):
        p = image_plan(int(h), int(w), tile_size)
        key = (p.Hp, p.Wp) if seeds is None else (p.Hp, p.Wp, int(seeds[i]))
        if key not in keys:
            keys.append(key)
            classes.append((p.Hp, p.Wp))
        plans.append(p._replace(noise_class=keys.index(key)))
    if seeds is None:
        return plans, classes
    return plans, classes, [k[2] for k in keys]


def even_step_tiles(h: int, w: int, tile_size: int = 256) -> int:
    """Tiles of an ``h x w`` image's even grid (the larger of its two grids)."""
    return len(image_plan(h, w, tile_size).coords0)


def plan_lockstep_groups(sizes: Sequence[Tuple[int, int]], tile_budget: int, tile_size: int = 256) -> List[List[int]]:
    """``--lockstep_tiles``: consecutive images (HR sizes, in file order) are grouped; a group closes before an image that
    would push its even-step tile count above ``tile_budget``, so an image larger than the budget runs alone.  Returns the
    groups as lists of indices into ``sizes``."""
    groups: List[List[int]] = []
    cur: List[int] = []
    cur_tiles = 0
    for i, (h, w) in enumerate(sizes):
        t = even_step_tiles(h, w, tile_size)
        if cur and cur_tiles + t > tile_budget:
            groups.append(cur)
            cur, cur_tiles = [], 0
        cur.append(i)
        cur_tiles += t
    if cur:
        groups.append(cur)
    return groups
