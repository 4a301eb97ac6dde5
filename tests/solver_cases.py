"""Yardsticks and inputs of the few-step sampler tests (tests/test_solver_cpu.py, tests/test_solver_gpu.py).

(a) ``levels`` / ``ddim64`` / ``ddpm64`` / ``weights64``: an independent float64 statement of the step tables and the 2M history
    weights from the fp32 log-SNR levels of a run.
(b) ``gain_error``: the closed-form case - for x0 ~ N(0, s^2) the ideal predictor is x0 = a s^2 / (a^2 s^2 + sg^2) x, every update is
    linear in x, and the deterministic samplers' exact end-to-end gain is the ratio of the marginals' standard deviations.
(c) ``history_np``: the history step of include/srgd_solver.h in numpy fp32 (bit for bit).
(d) ``solver_tiled_sample``: ``oracle.srgd_oracle.tiled_sample``'s loop restated from the oracle's own functions - per chunk
    ``O.predict_and_step`` gives x0, a ``NoiseSource`` that hands back its last draw gives z, the update is A x + B x0 + S z from (a),
    the guidance correction and then the history term follow the scatter.
The end-to-end cases share the inputs of tests/guidance_cases.py; the oracle runs are made once per session, read-only."""
import contextlib
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import srgd_oracle as O
from tests import guidance_cases as G

S_DATA = 0.5                                            # the standard deviation of x0 in the closed-form case
MAX_ABS = 1.5
SENTINEL = np.float32(-7.25e33)
KERNEL_WEIGHTS = [0.37, -1.25]


# ------------------------------------------------------------------------------------------- (a) tables in float64
def levels(n, spacing):
    """The N + 1 fp32 log-SNR levels of a run, 0-dim tensors."""
    if spacing == "logsnr":
        lv = torch.linspace(float(O.log_snr_linear(torch.tensor(1.0))), float(O.log_snr_linear(torch.tensor(0.0))), n + 1)
        assert lv.dtype == torch.float32
        return [lv[i] for i in range(n + 1)]
    steps = torch.linspace(1.0, 0.0, n + 1)
    return [O.log_snr_linear(steps[i]) for i in range(n + 1)]


def _marginal(l):
    """(alpha, sigma) of a log-SNR, float64."""
    l = float(l)
    return math.sqrt(1.0 / (1.0 + math.exp(-l))), math.sqrt(1.0 / (1.0 + math.exp(l)))


def ddpm64(l0, l1):
    """(A, B, S) of the reference's ancestral step (model.py:3164, :3168) in float64."""
    (a0, _), (a1, s1) = _marginal(l0), _marginal(l1)
    c = -math.expm1(float(l0) - float(l1))
    return a1 * (1.0 - c) / a0, a1 * c, math.sqrt(s1 * s1 * c)


def ddim64(l0, l1, eta):
    """(A, B, S) of the DDIM family's step in float64: x' = a' x0 + k (x - a x0) / s + eta s~ z."""
    (a0, s0), (a1, s1) = _marginal(l0), _marginal(l1)
    var = s1 * s1 * -math.expm1(float(l0) - float(l1))
    k = math.sqrt(s1 * s1 - eta * eta * var)
    return k / s0, a1 - k * a0 / s0, eta * math.sqrt(var)


def weights64(lv, first=0):
    """The 2M history weights B_i h_i / (2 h_{i-1}), zero on the first executed step, the last one and the skipped ones."""
    lv = [float(v) for v in lv]
    n = len(lv) - 1
    return [ddim64(lv[i], lv[i + 1], 0.0)[1] * (lv[i + 1] - lv[i]) / (2.0 * (lv[i] - lv[i - 1])) if first < i < n - 1 else 0.0
            for i in range(n)]


# ------------------------------------------------------------------------------------------- (b) the closed-form case
def gain_error(tables, weights, lv, s=S_DATA):
    """Relative error of the end-to-end gain of a linear run: ``tables`` [(A, B)] and ``weights`` per step, ``lv`` the levels."""
    x, prev = 1.0, 0.0
    for i, ((a_, b_), w) in enumerate(zip(tables, weights)):
        al, sg = _marginal(lv[i])
        x0 = al * s * s / (al * al * s * s + sg * sg) * x
        x = a_ * x + b_ * x0 + w * (x0 - prev)
        prev = x0
    (a0, s0), (a1, s1) = _marginal(lv[0]), _marginal(lv[-1])
    exact = math.sqrt((a1 * a1 * s * s + s1 * s1) / (a0 * a0 * s * s + s0 * s0))
    return abs(x / exact - 1.0)


# ------------------------------------------------------------------------------------------- (c) the kernel in numpy fp32
def history_np(img, xs, xp, recs, w):
    """include/srgd_solver.h on flat float32 arrays, in place on ``img`` and ``xp``: ``recs`` = [(canvas_off, Hp, Wp, top, left, h, w)]."""
    w32 = np.float32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        for (off, hp, wp, top, left, h, wd) in recs:
            box = (slice(None), slice(top, top + h), slice(left, left + wd))
            i_, s_, p_ = (a[off:off + 3 * hp * wp].reshape(3, hp, wp) for a in (img, xs, xp))
            d = s_[box] - p_[box]
            assert d.dtype == np.float32
            if w32 != 0:
                i_[box] = i_[box] + w32 * d
            p_[box] = s_[box]


def kernel_buffers(recs, seed, gaps=True):
    """(img, x_start, x_prev) flat float32 for a record list: uniform in [-1.5, 1.5] inside every canvas (boxes and the canaries
    around them), the sentinel between the canvases."""
    total = max(off + 3 * hp * wp for (off, hp, wp, *_r) in recs)
    rng = np.random.default_rng([seed, len(recs), total])
    out = []
    for _ in range(3):
        a = np.full(total, SENTINEL, dtype=np.float32)
        for (off, hp, wp, *_r) in recs:
            a[off:off + 3 * hp * wp] = rng.uniform(-MAX_ABS, MAX_ABS, 3 * hp * wp).astype(np.float32)
        out.append(a)
    return out


# 37 x 53 with the box 20 x 31 at (3, 5); two sizes at non-zero offsets, then a canvas whose rows begin on 16-byte boundaries (the
# four-dword form of the kernel, with a row tail of one) behind them; 130 images: the 128-image launch limit is crossed
KERNEL_GROUPS = {
    "solo": [(0, 37, 53, 3, 5, 20, 31)],
    "group": [(7, 19, 23, 1, 3, 15, 17), (7 + 3 * 19 * 23 + 5, 41, 29, 7, 1, 33, 27), (2 * 4096, 24, 40, 3, 4, 13, 29)],
    "many": [(k * (3 * 64 + 3), 8, 8, 1, 1, 6, 6) for k in range(130)],
}


# ------------------------------------------------------------------------------------------- (d) the restated loop
class LastDraw(O.NoiseSource):
    """Draws as ``NoiseSource`` does and keeps the last draw."""
    last = None

    def randn(self, shape):
        self.last = super().randn(shape)
        return self.last


@contextlib.contextmanager
def levels_as_times():
    """Inside, the oracle's schedule takes the 'time' it is handed for the log-SNR itself: ``O.predict_and_step(..., t=level, ...)``
    conditions the U-Net on that level and forms x0 with its alpha and sigma."""
    saved = O.log_snr_linear
    O.log_snr_linear = lambda t: t
    try:
        yield
    finally:
        O.log_snr_linear = saved


def solver_tiled_sample(sd, cfg, condition_x, class_label=None, *, sampler="ddpm", eta=None, step_spacing="time",
                        consistency_guidance=0.0, consistency_guidance_start_steps=0, batch_size=4, num_sample_steps=50,
                        cond_scale=1.0, guidance_start_steps=0, class_cond_scale=1.0, class_guidance_start_steps=0, tile=256,
                        generation_start_steps=0, start_white_noise=True, noise=None, trace=None):
    """``O.tiled_sample`` with the step A x + B x0 + S z of the sampler, the LR-consistency correction and the 2M history term."""
    noise = noise or LastDraw()
    n = num_sample_steps
    lv = levels(n, step_spacing)
    if sampler == "ddpm":
        tables = [ddpm64(lv[i], lv[i + 1]) for i in range(n)]
    else:
        tables = [ddim64(lv[i], lv[i + 1], float(eta or 0.0)) for i in range(n)]
    wts = weights64(lv, generation_start_steps) if sampler == "dpmpp2m" else [0.0] * n
    cond = condition_x * 2 - 1
    target = cond.clone()
    _, _, h, w = cond.shape
    (left, top, right, bottom), pad = O.canvas_box_and_pad(h, w)
    cond = F.pad(cond, pad, mode="reflect")
    if generation_start_steps > 0 or not start_white_noise:
        if step_spacing == "logsnr":
            ls0 = lv[generation_start_steps]
        else:
            ls0 = O.log_snr_linear((1.0 - torch.tensor(generation_start_steps / n)) if generation_start_steps > 0 else torch.tensor(1.0))
        img = cond * ls0.sigmoid().sqrt() + noise.randn(cond.shape) * (-ls0).sigmoid().sqrt()
    else:
        img = noise.randn(cond.shape)
    hp, wp = cond.shape[-2:]
    grids = O.sampling_grids(hp, wp, tile, tile)
    (il, it, ir, ib), ipad = O.grid_bbox(grids[1], hp, wp)
    cond = F.pad(cond[:, :, it:ib, il:ir], ipad, mode="constant", value=0.0)
    x_start = img.clone()
    x_prev = x_start.clone()
    for i in range(n):
        if i < generation_start_steps:
            continue
        cs = cond_scale if i >= guidance_start_steps else 1.0
        ccs = class_cond_scale if i >= class_guidance_start_steps else 1.0
        last = i == n - 1
        a_, b_, s_ = tables[i]
        boxes = grids[i % 2]
        for j in range(0, len(boxes), batch_size):
            chunk = boxes[j:j + batch_size]
            xb = torch.cat([img[:, :, a:b, c:d] for (a, b, c, d) in chunk], dim=0)
            cb = torch.cat([cond[:, :, a:b, c:d] for (a, b, c, d) in chunk], dim=0)
            with levels_as_times():                      # x0 of the level; the oracle's own update is not used
                _, x0 = O.predict_and_step(sd, cfg, xb, lv[i], torch.tensor(0.0) if last else lv[i + 1], cb, class_label, cs, ccs,
                                           noise, trace)
            out = a_ * xb.double() + b_ * x0.double()
            if not last:                                 # the draw a ddpm step makes, whatever its scale
                out = out + s_ * noise.last.double()
            out = out.float()
            for k, (a, b, c, d) in enumerate(chunk):
                img[:, :, a:b, c:d] = out[k]
                x_start[:, :, a:b, c:d] = x0[k]
        if consistency_guidance > 0 and i >= consistency_guidance_start_steps:
            g = target - torch.from_numpy(G.ud64(x_start[:, :, top:bottom, left:right].numpy())).to(torch.float32)
            x_start[:, :, top:bottom, left:right] += consistency_guidance * g
            img[:, :, top:bottom, left:right] += (consistency_guidance * b_) * g
        if sampler == "dpmpp2m":                         # after the correction: the history holds the corrected predictions
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


# the end-to-end cases: the shapes, steps, seeds and class guidance of tests/guidance_cases.py's
E2E_CASES = {
    "tile256_ddim0": dict(base="tile256", sampler="ddim", eta=0.0, step_spacing="time", weight=0.0, start=0),
    "tile256_ddim05": dict(base="tile256", sampler="ddim", eta=0.5, step_spacing="time", weight=0.0, start=0),
    "tile256_2m": dict(base="tile256", sampler="dpmpp2m", eta=None, step_spacing="logsnr", weight=0.0, start=0),
    "geo300_2m_guided": dict(base="geo300", sampler="dpmpp2m", eta=None, step_spacing="logsnr", weight=0.5, start=2),
}


def sampler_kw(name):
    case = E2E_CASES[name]
    kw = dict(sampler=case["sampler"], step_spacing=case["step_spacing"])
    if case["eta"] is not None:
        kw["eta"] = case["eta"]
    if case["weight"]:
        kw.update(consistency_guidance=case["weight"], consistency_guidance_start_steps=case["start"])
    return kw


@functools.lru_cache(maxsize=None)
def e2e_oracle(name):
    """(output [1,3,H,W], trace {"img", "x_start"}) of the restated loop on a case.  Host noise after ``torch.manual_seed(seed)``;
    the caller's generator is restored."""
    case = E2E_CASES[name]
    base = G.E2E_CASES[case["base"]]
    _, cond = G.e2e_input(case["base"])
    state = torch.get_rng_state()
    torch.manual_seed(base["seed"])
    trace = {}
    with torch.inference_mode():
        out = solver_tiled_sample(O.strip_model_prefix(G.state_dict()), O.UnetCfg(dim=G.DIM), cond, torch.tensor([G.LABEL]),
                                  batch_size=base["batch_size"], num_sample_steps=base["steps"],
                                  class_cond_scale=base["class_cond_scale"], trace=trace, **sampler_kw(name))
    torch.set_rng_state(state)
    return out, {k: v for k, v in trace.items() if k in ("img", "x_start")}
