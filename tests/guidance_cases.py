"""Yardsticks and inputs of the LR-consistency guidance tests (tests/test_guidance_cpu.py, tests/test_guidance_gpu.py).

(a) ``ud64``: U(D(X)) of include/srgd_guidance.h in float64 numpy - the rows of ``oracle.pil_resample.precompute_coeffs`` divided by
    2^22, laid into one matrix per pass; ``guide64`` is the whole step on a pair of canvases.
(b) ``guided_tiled_sample``: ``oracle.srgd_oracle.tiled_sample``'s loop restated from the oracle's own functions with the correction
    added after the scatter of each step; with a weight of 0 it is the oracle's loop line for line.
The end-to-end cases, their inputs (a smooth low-resolution image enlarged by Pillow: the condition the front end makes) and the
oracle runs are made once per session and shared, read-only."""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pil_resample as PR
from oracle import srgd_oracle as O
from srgd_amd.synth import synth_state_dict
from tests import consistency_cases as K

UNIT = 1.0 / (1 << PR.PRECISION_BITS)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 16
# the kernel tests: LR sizes (h, w) - 5x5: every index a border row or the single interior one; 16x23: one partial tile row of two
# tiles' height, odd width; 65x70: five tile rows and three tile columns, partial in both directions (canvas 768)
KERNEL_SIZES = [(5, 5), (16, 23), (65, 70)]
WEIGHTS = [(1.0, 0.37), (0.5, 1.0)]
MAX_ABS = 1.5
# fp32 accumulation: 4 passes x 17 roundings (16 taps and the store) x 2^-24 x sum|k| (1.24 at most; 1.4 is taken) x max|x|; the bar
# is 4 x that
KERNEL_BAR = 4 * (4 * 17 * 2.0 ** -24 * 1.4 * MAX_ABS)
SENTINEL = np.float32(-7.25e33)


@functools.lru_cache(maxsize=None)
def matrices(n):
    """(Dm [n, 4n], Um [4n, n]) float64: the reduction and the enlargement of a line of 4n / n samples."""
    bounds, kk = PR.precompute_coeffs(4 * n, n)
    down = np.zeros((n, 4 * n))
    for i in range(n):
        down[i, bounds[i, 0]:bounds[i, 0] + bounds[i, 1]] = kk[i, :bounds[i, 1]].astype(np.float64) * UNIT
    bounds, kk = PR.precompute_coeffs(n, 4 * n)
    up = np.zeros((4 * n, n))
    for j in range(4 * n):
        up[j, bounds[j, 0]:bounds[j, 0] + bounds[j, 1]] = kk[j, :bounds[j, 1]].astype(np.float64) * UNIT
    down.setflags(write=False)
    up.setflags(write=False)
    return down, up


def d64(x):
    """D(X): [..., 4h, 4w] -> [..., h, w], horizontal then vertical, float64."""
    x = np.asarray(x, dtype=np.float64)
    dh, dw = matrices(x.shape[-2] // 4)[0], matrices(x.shape[-1] // 4)[0]
    return dh @ (x @ dw.T)


def u64(d):
    """U(D): [..., h, w] -> [..., 4h, 4w], horizontal then vertical, float64."""
    d = np.asarray(d, dtype=np.float64)
    uh, uw = matrices(d.shape[-2])[1], matrices(d.shape[-1])[1]
    return uh @ (d @ uw.T)


def ud64(x):
    return u64(d64(x))


def geometry(h, w):
    """(Hp, Wp, top, left) of an LR size: ``get_coord_and_pad`` of its x4 output."""
    (left, top, _, _), pad = O.canvas_box_and_pad(4 * h, 4 * w)
    return 4 * h + pad[2] + pad[3], 4 * w + pad[0] + pad[1], top, left


def guide64(img, xs, cond01, top, left, weight_x0, weight_img):
    """The step of include/srgd_guidance.h on float32 canvases [3,Hp,Wp] and a condition [3,H,W] -> (img', x_start') float64."""
    hh, ww = cond01.shape[-2:]
    box = (slice(None), slice(top, top + hh), slice(left, left + ww))
    img2, xs2 = img.astype(np.float64), xs.astype(np.float64)
    with np.errstate(invalid="ignore"):
        g = (2.0 * cond01.astype(np.float64) - 1.0) - ud64(xs[box])
    xs2[box] += float(np.float32(weight_x0)) * g
    img2[box] += float(np.float32(weight_img)) * g
    return img2, xs2


@functools.lru_cache(maxsize=None)
def kernel_case(h, w, seed=0):
    """(img, x_start [3,Hp,Wp] float32: uniform in [-1.5, 1.5] inside the crop box, the sentinel outside; cond01 [3,4h,4w] in [0,1];
    (Hp, Wp, top, left)) - read-only."""
    hp, wp, top, left = geometry(h, w)
    rng = np.random.default_rng([seed, h, w])
    canv = []
    for _ in range(2):
        a = np.full((3, hp, wp), SENTINEL, dtype=np.float32)
        a[:, top:top + 4 * h, left:left + 4 * w] = rng.uniform(-MAX_ABS, MAX_ABS, (3, 4 * h, 4 * w)).astype(np.float32)
        a.setflags(write=False)
        canv.append(a)
    cond = rng.random((3, 4 * h, 4 * w), dtype=np.float32)
    cond.setflags(write=False)
    return canv[0], canv[1], cond, (hp, wp, top, left)


# ------------------------------------------------------------------------------------------- (b) the guided oracle
def smooth_lr(h, w, seed):
    """A smooth uint8 [h,w,3] low-resolution image with a little texture."""
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng([seed, h, w])
    base = np.stack([128 + 90 * np.sin(x / 7.0 + seed) * np.cos(y / 9.0), 110 + 1.2 * x - 0.7 * y, 140 + 60 * np.cos((x + y) / 11.0)], axis=2)
    return np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)


def condition_of(lr):
    """The condition the front end makes of an input: Pillow x4, / 255 -> float32 tensor [1,3,4h,4w]."""
    return torch.from_numpy(np.ascontiguousarray((K.pillow_up(lr).astype(np.float32) / np.float32(255)).transpose(2, 0, 1)))[None]


def lr_mse(out01, lr):
    """LR-MSE of an output [1,3,H,W] in [0,1] as saved (mul 255, truncation) against its input, by tests/consistency_cases.py."""
    return K.yardstick(np.ascontiguousarray(PR.to_u8_hwc(out01[0].cpu().numpy())), lr)[2]["lr_mse"]


def guided_tiled_sample(sd, cfg, condition_x, class_label=None, *, consistency_guidance=0.0, consistency_guidance_start_steps=0,
                        batch_size=4, num_sample_steps=50, cond_scale=1.0, guidance_start_steps=0, class_cond_scale=1.0,
                        class_guidance_start_steps=0, tile=256, generation_start_steps=0, start_white_noise=True, noise=None,
                        trace=None):
    """``O.tiled_sample`` with the LR-consistency correction after the scatter of each guided step."""
    noise = noise or O.NoiseSource()
    cond = condition_x * 2 - 1
    target = cond.clone()                                                # C = 2 cond01 - 1
    _, _, h, w = cond.shape
    (left, top, right, bottom), pad = O.canvas_box_and_pad(h, w)
    cond = F.pad(cond, pad, mode="reflect")
    if generation_start_steps > 0 or not start_white_noise:
        t0 = (1.0 - torch.tensor(generation_start_steps / num_sample_steps)) if generation_start_steps > 0 else torch.tensor(1.0)
        ls0 = O.log_snr_linear(t0)
        img = cond * ls0.sigmoid().sqrt() + noise.randn(cond.shape) * (-ls0).sigmoid().sqrt()
    else:
        img = noise.randn(cond.shape)
    steps = torch.linspace(1.0, 0.0, num_sample_steps + 1)
    hp, wp = cond.shape[-2:]
    grids = O.sampling_grids(hp, wp, tile, tile)
    (il, it, ir, ib), ipad = O.grid_bbox(grids[1], hp, wp)
    cond = F.pad(cond[:, :, it:ib, il:ir], ipad, mode="constant", value=0.0)
    x_start = img.clone()
    for i in range(num_sample_steps):
        if i < generation_start_steps:
            continue
        cs = cond_scale if i >= guidance_start_steps else 1.0
        ccs = class_cond_scale if i >= class_guidance_start_steps else 1.0
        t, t_next = steps[i], steps[i + 1]
        boxes = grids[i % 2]
        for j in range(0, len(boxes), batch_size):
            chunk = boxes[j:j + batch_size]
            xb = torch.cat([img[:, :, a:b, c:d] for (a, b, c, d) in chunk], dim=0)
            cb = torch.cat([cond[:, :, a:b, c:d] for (a, b, c, d) in chunk], dim=0)
            out, x0 = O.predict_and_step(sd, cfg, xb, t, t_next, cb, class_label, cs, ccs, noise, trace)
            for k, (a, b, c, d) in enumerate(chunk):
                img[:, :, a:b, c:d] = out[k]
                x_start[:, :, a:b, c:d] = x0[k]
        if consistency_guidance > 0 and i >= consistency_guidance_start_steps:      # the correction: the posterior mean is linear in x0
            s = O.step_scalars(t, t_next)
            g = target - torch.from_numpy(ud64(x_start[:, :, top:bottom, left:right].numpy())).to(torch.float32)
            x_start[:, :, top:bottom, left:right] += consistency_guidance * g
            img[:, :, top:bottom, left:right] += consistency_guidance * (s["alpha_next"] * s["c"]) * g
        if i % 2 == 1:
            inner = img[:, :, it:ib, il:ir].clone()
            sigma = (-O.log_snr_linear(t_next)).sigmoid().sqrt()
            img = noise.randn(cond.shape) * sigma
            img[:, :, it:ib, il:ir] = inner
        if trace is not None:
            trace.setdefault("img", []).append(img.clone())
            trace.setdefault("x_start", []).append(x_start.clone())
    out = img[:, :, top:bottom, left:right].clamp(-1.0, 1.0)
    return (out + 1) * 0.5


# the end-to-end cases: one 256^2 tile, 6 steps (each parity's step graph runs eager, captured and replayed), weight 1;
# the 300x300 geometry (9 / 4 tiles), 4 steps, weight 0.5 from step 2 on, under class guidance 2.0
E2E_CASES = {
    "tile256": dict(lr=(64, 64), steps=6, weight=1.0, start=0, class_cond_scale=1.0, batch_size=4, seed=71, lr_seed=1),
    "geo300": dict(lr=(75, 75), steps=4, weight=0.5, start=2, class_cond_scale=2.0, batch_size=4, seed=71, lr_seed=2),
}
LABEL = 0


@functools.lru_cache(maxsize=None)
def state_dict():
    with open(os.path.join(ROOT, "tests", "golden", f"schema_dim{DIM}.json")) as f:
        schema = {k: tuple(v) for k, v in json.load(f).items()}
    return synth_state_dict(schema, seed=0)


@functools.lru_cache(maxsize=None)
def e2e_input(name):
    """(lr uint8 [h,w,3], condition [1,3,4h,4w] float32) of a case."""
    case = E2E_CASES[name]
    lr = smooth_lr(*case["lr"], case["lr_seed"])
    lr.setflags(write=False)
    return lr, condition_of(lr)


@functools.lru_cache(maxsize=None)
def e2e_oracle(name, guided):
    """(output [1,3,H,W], trace {"img": [...], "x_start": [...]}) of the CPU oracle on a case: ``guided`` - the restated loop with the
    case's weight, else ``O.tiled_sample`` itself.  Host noise after ``torch.manual_seed(seed)``; the caller's generator is restored."""
    case = E2E_CASES[name]
    _, cond = e2e_input(name)
    state = torch.get_rng_state()
    torch.manual_seed(case["seed"])
    trace = {}
    kw = dict(batch_size=case["batch_size"], num_sample_steps=case["steps"], class_cond_scale=case["class_cond_scale"], trace=trace)
    with torch.inference_mode():
        if guided:
            out = guided_tiled_sample(O.strip_model_prefix(state_dict()), O.UnetCfg(dim=DIM), cond, torch.tensor([LABEL]),
                                      consistency_guidance=case["weight"], consistency_guidance_start_steps=case["start"], **kw)
        else:
            out = O.tiled_sample(O.strip_model_prefix(state_dict()), O.UnetCfg(dim=DIM), cond, torch.tensor([LABEL]), **kw)
    torch.set_rng_state(state)
    return out, {k: v for k, v in trace.items() if k in ("img", "x_start")}
