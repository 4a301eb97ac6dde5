"""Yardsticks and inputs of the dynamic-threshold tests (tests/test_threshold_cpu.py, tests/test_threshold_gpu.py).

(a) ``position_np`` / ``select_np`` / ``threshold_np``: include/srgd_threshold.h restated in numpy fp32 - the keys, the position, the
    threshold and the update, in place on flat float32 arrays.
(b) ``buffers`` and ``KERNEL_CASES``: sentinel-filled flat buffers with every canvas at a non-zero offset and canaries between the
    canvases, and the table of kernel cases - each a function of the implementation's chunk size that returns
    ``(records, img, x_start, q)``.
(c) ``thresholded_tiled_sample``: ``oracle.srgd_oracle.tiled_sample``'s loop restated as tests/solver_cases.py restates it, with the
    unclamped prediction x0 = (x - sigma eps) / alpha formed from the ``eps`` the oracle's ``predict_and_step`` records, all tiles of a
    step scattered first, then s per image, then the update; the guidance correction and the history term follow.
The end-to-end cases share the inputs of tests/guidance_cases.py; the oracle runs are made once per session, read-only."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import srgd_oracle as O
from tests import guidance_cases as G
from tests import solver_cases as SC

SENTINEL = np.float32(-7.25e33)
WEIGHT = 0.37
QS = [float(np.float32(0.5)), float(np.float32(0.9)), float(np.float32(0.995)), 1.0, float(np.float32(1e-7))]
P = 0.995


# ------------------------------------------------------------------------------------------- (a) the definition in numpy fp32
def keys_of(a):
    """key(v): the bit pattern with the sign bit cleared, uint32."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def position_np(n, q):
    """(lo, hi, frac): pos = (double) q * (double) (n - 1) of the fp32 q; Python's float is the double."""
    pos = float(np.float32(q)) * float(n - 1)
    lo = math.floor(pos)
    return lo, min(lo + 1, n - 1), np.float32(pos - lo)


def select_np(values, q):
    """(a_lo, a_hi, s_raw, s) of the values of a statistics box, float32: the two order statistics by ``np.partition`` on the keys."""
    k = keys_of(values).reshape(-1)
    lo, hi, frac = position_np(k.size, q)
    part = np.partition(k, sorted({lo, hi}))
    a_lo, a_hi = part[lo:lo + 1].view(np.float32)[0], part[hi:hi + 1].view(np.float32)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.float32(a_hi - a_lo)
        prod = np.float32(frac * diff)
        s_raw = np.float32(a_lo + prod)
    s = np.float32(1.0) if s_raw < 1 else s_raw
    return a_lo, a_hi, s_raw, s


def canvas(a, rec):
    """The [3, Hp, Wp] view of a record's canvas in a flat array."""
    off, hp, wp = rec[:3]
    return a[off:off + 3 * hp * wp].reshape(3, hp, wp)


def stats_box(a, rec):
    _, _, _, top, left, h, w = rec[:7]
    return canvas(a, rec)[:, top:top + h, left:left + w]


def update_box(a, rec):
    bt, bl, bh, bw = rec[7:]
    return canvas(a, rec)[:, bt:bt + bh, bl:bl + bw]


def threshold_np(img, xs, recs, q, weight):
    """The call in place on flat float32 ``img`` and ``xs``; ``recs`` = [(canvas_off, Hp, Wp, top, left, H, W, box_t, box_l, box_h,
    box_w)].  -> float32 array of every image's s."""
    w32 = np.float32(weight)
    out = np.empty(len(recs), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for i, rec in enumerate(recs):
            s = select_np(stats_box(xs, rec), q)[3]
            out[i] = s
            xb, ib = update_box(xs, rec), update_box(img, rec)
            v = xb.copy()
            t = np.where(v < -s, -s, np.where(v > s, s, v)).astype(np.float32)
            y = (t / s).astype(np.float32)
            d = (y - v).astype(np.float32)
            xb[...] = y
            m = d != 0
            ib[m] = (ib[m] + (w32 * d[m]).astype(np.float32)).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------- (b) buffers and the kernel cases
def buffers(recs, seed, scale=1.5):
    """(img, x_start) flat float32 for a record list: uniform in [-scale, scale] inside every canvas, the sentinel between them."""
    total = max(r[0] + 3 * r[1] * r[2] for r in recs) + 7
    rng = np.random.default_rng([seed, len(recs), total])
    out = []
    for _ in range(2):
        a = np.full(total, SENTINEL, dtype=np.float32)
        for r in recs:
            a[r[0]:r[0] + 3 * r[1] * r[2]] = rng.uniform(-scale, scale, 3 * r[1] * r[2]).astype(np.float32)
        out.append(a)
    return out


NESTED = (5, 13, 16, 4, 5, 5, 7, 2, 3, 9, 11)           # a 5 x 7 statistics box in a 9 x 11 update box in a 13 x 16 canvas: N = 105


def _fill(xs, rec, values, seed):
    """The statistics box of ``rec`` = the given N values in a shuffled order."""
    box = stats_box(xs, rec)
    v = np.asarray(values, dtype=np.float32).copy()
    assert v.size == box.size
    np.random.default_rng(seed).shuffle(v)
    box[...] = v.reshape(box.shape)


def _nested(seed, q, values=None):
    recs = [NESTED]
    img, xs = buffers(recs, seed)
    if values is not None:
        _fill(xs, NESTED, values, seed)
    return recs, img, xs, q


def case_nested_huge(chunk):
    """Huge values in the update box outside the statistics box: they do not move s, and they are thresholded."""
    recs, img, xs, q = _nested(1, 0.9)
    keep = stats_box(xs, NESTED).copy()
    update_box(xs, NESTED)[...] = np.where(np.arange(3 * 9 * 11).reshape(3, 9, 11) % 2 == 0, np.float32(3e30), np.float32(-7e8))
    stats_box(xs, NESTED)[...] = keep
    return recs, img, xs, q


def _sized(h, w, seed, q=P):
    recs = [(3, h + 3, w + 5, 2, 1, h, w, 1, 0, h + 2, w + 4)]
    img, xs = buffers(recs, seed)
    return recs, img, xs, q


# N = 3 H W is a multiple of 3 and the chunk a power of two, so N = chunk and N = chunk + 1 do not exist: the three sizes around a chunk
# boundary are chunk - 1 (one workgroup, its last key missing), 3 chunks exactly (the last workgroup full) and 2 chunks + 1 (a workgroup of
# one key) - each of the three remainders 4095, 0 and 1 the issue asks for
def case_chunk_minus_1(chunk):
    assert (chunk - 1) % 3 == 0
    n = (chunk - 1) // 3
    h = next(d for d in range(int(math.isqrt(n)), 0, -1) if n % d == 0)
    return _sized(h, n // h, 2)


def case_chunks_exactly(chunk):
    h = 1 << (int(math.log2(chunk)) // 2)
    assert chunk % h == 0
    return _sized(h, chunk // h, 3)


def case_chunks_plus_1(chunk):
    assert (2 * chunk + 1) % 3 == 0
    n = (2 * chunk + 1) // 3
    h = next(d for d in range(int(math.isqrt(n)), 0, -1) if n % d == 0)
    return _sized(h, n // h, 4)


def case_all_equal(chunk):
    return _nested(5, P, np.full(105, 1.75))


def case_two_values(chunk):
    """q = 0.9 of 105: pos 93.6 - 94 values of 1.25 (ranks 0 .. 93), 11 of 2.5: lo and hi on either side."""
    lo, hi, _ = position_np(105, 0.9)
    assert (lo, hi) == (93, 94)
    return _nested(6, 0.9, [1.25] * 94 + [-2.5] * 11)


def case_low_bits(chunk):
    """Values that differ in the lowest 10 mantissa bits only: the last pass decides."""
    rng = np.random.default_rng(7)
    bits = (np.uint32(0x3FC00000) + rng.integers(0, 1024, 105).astype(np.uint32)) | (rng.integers(0, 2, 105).astype(np.uint32) << np.uint32(31))
    return _nested(7, 0.9, bits.view(np.float32))


def case_middle_bits(chunk):
    """Values that differ in mantissa bits 10 .. 19 only: the second pass decides."""
    rng = np.random.default_rng(8)
    bits = np.uint32(0x3FC00000) + (rng.integers(0, 1024, 105).astype(np.uint32) << np.uint32(10))
    return _nested(8, 0.9, bits.view(np.float32))


def case_sign_only(chunk):
    return _nested(9, 0.9, np.where(np.arange(105) % 3 == 0, 1.5, -1.5))


def case_zeros_and_denormals(chunk):
    """+0, -0 and denormals of both signs: the assertion is on s only (it is 1)."""
    rng = np.random.default_rng(10)
    bits = rng.integers(0, 1 << 23, 105).astype(np.uint32) | (rng.integers(0, 2, 105).astype(np.uint32) << np.uint32(31))
    bits[:20] &= np.uint32(0x80000000)
    return _nested(10, 0.9, bits.view(np.float32))


def case_quantile_below_1(chunk):
    """The median of uniform(-1.5, 1.5) magnitudes is 0.75: s is exactly 1."""
    return _nested(11, 0.5)


def case_q_one(chunk):
    return _nested(12, 1.0)


def case_frac_zero(chunk):
    lo, hi, frac = position_np(105, 0.5)
    assert (lo, hi, float(frac)) == (52, 53, 0.0)
    recs, img, xs, q = _nested(13, 0.5)
    xs *= np.where(xs == SENTINEL, np.float32(1), np.float32(2))         # magnitudes up to 3: the median exceeds 1
    return recs, img, xs, q


THREE = [(7, 19, 23, 3, 4, 13, 15, 1, 3, 15, 17), (7 + 3 * 19 * 23 + 5, 41, 80, 7, 2, 33, 70, 7, 1, 34, 72),
         (3 * 4096, 100, 50, 2, 3, 91, 45, 0, 0, 100, 50)]


def case_three_sizes(chunk):
    img, xs = buffers(THREE, 14)
    return THREE, img, xs, P


def case_many(chunk):
    """130 images of 8 x 8: the 128-image launch limit is crossed."""
    recs = [(k * (3 * 64 + 3) + 1, 8, 8, 1, 1, 6, 6, 0, 0, 8, 8) for k in range(130)]
    img, xs = buffers(recs, 15, scale=2.5)
    return recs, img, xs, 0.9


def case_one_nan_above(chunk):
    recs, img, xs, q = _nested(16, 0.9)
    stats_box(xs, NESTED)[1, 2, 3] = np.nan
    return recs, img, xs, q


def case_nans_reach_hi(chunk):
    """12 NaNs of 105 at q = 0.9: ranks 93 .. 104 are NaN, hi = 94."""
    recs, img, xs, q = _nested(17, 0.9)
    box = stats_box(xs, NESTED)
    for e in range(5, 101, 8):                           # 12 elements
        box[e // 35, (e % 35) // 7, e % 7] = np.nan
    assert int(np.isnan(stats_box(xs, NESTED)).sum()) == 12
    return recs, img, xs, q


def case_inf_at_the_rank(chunk):
    """11 infinities of 105 at q = 0.9: a_lo is finite, a_hi = +Inf."""
    recs, img, xs, q = _nested(18, 0.9)
    box = stats_box(xs, NESTED)
    for e in range(3, 105, 10):                          # 11 elements
        box[e // 35, (e % 35) // 7, e % 7] = np.float32(-np.inf if e > 3 else np.inf)
    assert int(np.isinf(stats_box(xs, NESTED)).sum()) == 11
    return recs, img, xs, q


KERNEL_CASES = {f.__name__[5:]: f for f in (
    case_nested_huge, case_chunk_minus_1, case_chunks_exactly, case_chunks_plus_1, case_all_equal, case_two_values, case_low_bits,
    case_middle_bits, case_sign_only, case_quantile_below_1, case_q_one, case_frac_zero, case_three_sizes, case_many,
    case_one_nan_above, case_nans_reach_hi, case_inf_at_the_rank)}


# ------------------------------------------------------------------------------------------- (c) the restated loop
def thresholded_tiled_sample(sd, cfg, condition_x, class_label=None, *, dynamic_threshold, sampler="ddpm", eta=None, step_spacing="time",
                             consistency_guidance=0.0, consistency_guidance_start_steps=0, batch_size=4, num_sample_steps=50,
                             cond_scale=1.0, guidance_start_steps=0, class_cond_scale=1.0, class_guidance_start_steps=0, tile=256,
                             generation_start_steps=0, noise=None, trace=None):
    """tests/solver_cases.py's ``solver_tiled_sample`` with the unclamped prediction and the dynamic threshold after the scatter of
    every step, before the guidance correction and the history term.  ``trace`` gains "s": every executed step's s."""
    noise = noise or SC.LastDraw()
    n = num_sample_steps
    lv = SC.levels(n, step_spacing)
    if sampler == "ddpm":
        tables = [SC.ddpm64(lv[i], lv[i + 1]) for i in range(n)]
    else:
        tables = [SC.ddim64(lv[i], lv[i + 1], float(eta or 0.0)) for i in range(n)]
    wts = SC.weights64(lv, generation_start_steps) if sampler == "dpmpp2m" else [0.0] * n
    cond = condition_x * 2 - 1
    target = cond.clone()
    _, _, h, w = cond.shape
    (left, top, right, bottom), pad = O.canvas_box_and_pad(h, w)
    cond = F.pad(cond, pad, mode="reflect")
    assert generation_start_steps == 0
    img = noise.randn(cond.shape)
    hp, wp = cond.shape[-2:]
    grids = O.sampling_grids(hp, wp, tile, tile)
    (il, it, ir, ib), ipad = O.grid_bbox(grids[1], hp, wp)
    cond = F.pad(cond[:, :, it:ib, il:ir], ipad, mode="constant", value=0.0)
    x_start = img.clone()
    x_prev = x_start.clone()
    for i in range(n):
        cs = cond_scale if i >= guidance_start_steps else 1.0
        ccs = class_cond_scale if i >= class_guidance_start_steps else 1.0
        last = i == n - 1
        a_, b_, s_ = tables[i]
        boxes = grids[i % 2]
        for j in range(0, len(boxes), batch_size):
            chunk = boxes[j:j + batch_size]
            xb = torch.cat([img[:, :, a:b, c:d] for (a, b, c, d) in chunk], dim=0)
            cb = torch.cat([cond[:, :, a:b, c:d] for (a, b, c, d) in chunk], dim=0)
            rec = {}
            with SC.levels_as_times():                   # eps of the level; x0 without the oracle's clamp
                level_next = torch.tensor(0.0) if last else lv[i + 1]
                O.predict_and_step(sd, cfg, xb, lv[i], level_next, cb, class_label, cs, ccs, noise, rec)
                sc = O.step_scalars(lv[i], level_next)
            x0 = (xb - sc["sigma"] * rec["eps"][-1]) / sc["alpha"]
            out = a_ * xb.double() + b_ * x0.double()
            if not last:                                 # the draw a ddpm step makes, whatever its scale
                out = out + s_ * noise.last.double()
            out = out.float()
            for k, (a, b, c, d) in enumerate(chunk):
                img[:, :, a:b, c:d] = out[k]
                x_start[:, :, a:b, c:d] = x0[k]
        # the dynamic threshold: s of the crop box, the update on what the step wrote
        s = float(select_np(x_start[0, :, top:bottom, left:right].numpy(), dynamic_threshold)[3])
        ut, ub, ul, ur = (0, hp, 0, wp) if i % 2 == 0 else (it, ib, il, ir)
        v = x_start[:, :, ut:ub, ul:ur].clone()
        y = v.clamp(-s, s) / s
        x_start[:, :, ut:ub, ul:ur] = y
        img[:, :, ut:ub, ul:ur] += (b_ * (y - v).double()).float()
        if trace is not None:
            trace.setdefault("s", []).append(s)
        if consistency_guidance > 0 and i >= consistency_guidance_start_steps:
            g = target - torch.from_numpy(G.ud64(x_start[:, :, top:bottom, left:right].numpy())).to(torch.float32)
            x_start[:, :, top:bottom, left:right] += consistency_guidance * g
            img[:, :, top:bottom, left:right] += (consistency_guidance * b_) * g
        if sampler == "dpmpp2m":                         # after the corrections: the history holds the corrected predictions
            d_ = x_start[:, :, it:ib, il:ir] - x_prev[:, :, it:ib, il:ir]
            img[:, :, it:ib, il:ir] += wts[i] * d_
            x_prev[:, :, it:ib, il:ir] = x_start[:, :, it:ib, il:ir]
        if i % 2 == 1:
            inner = img[:, :, it:ib, il:ir].clone()
            sigma = (-lv[i + 1]).sigmoid().sqrt()
            img = noise.randn(cond.shape) * sigma
            img[:, :, it:ib, il:ir] = inner
        if trace is not None:
            trace.setdefault("img", []).append(img.clone())
            trace.setdefault("x_start", []).append(x_start.clone())
    out = img[:, :, top:bottom, left:right].clamp(-1.0, 1.0)
    return (out + 1) * 0.5


# one 256^2 tile, 4 steps, class guidance 2.0; the 300x300 geometry (9 / 4 tiles, the crop box inside the inner box), dpmpp2m on the
# log-SNR grid with the LR-consistency guidance at 0.5
E2E_CASES = {
    "tile256": dict(base="tile256", steps=4, class_cond_scale=2.0, kw=dict()),
    "geo300_2m_guided": dict(base="geo300", steps=4, class_cond_scale=2.0,
                             kw=dict(sampler="dpmpp2m", step_spacing="logsnr", consistency_guidance=0.5)),
}


@functools.lru_cache(maxsize=None)
def e2e_oracle(name):
    """(output [1,3,H,W], trace {"img", "x_start", "s"}) of the restated loop on a case.  Host noise after ``torch.manual_seed(seed)``;
    the caller's generator is restored.  The case's condition: the restatement's own s exceeds 1 on the first executed step."""
    case = E2E_CASES[name]
    base = G.E2E_CASES[case["base"]]
    _, cond = G.e2e_input(case["base"])
    state = torch.get_rng_state()
    torch.manual_seed(base["seed"])
    trace = {}
    with torch.inference_mode():
        out = thresholded_tiled_sample(O.strip_model_prefix(G.state_dict()), O.UnetCfg(dim=G.DIM), cond, torch.tensor([G.LABEL]),
                                       dynamic_threshold=P, batch_size=base["batch_size"], num_sample_steps=case["steps"],
                                       class_cond_scale=case["class_cond_scale"], trace=trace, **case["kw"])
    torch.set_rng_state(state)
    assert trace["s"][0] > 1.0, trace["s"]
    return out, trace
