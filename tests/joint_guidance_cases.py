"""Yardsticks and inputs of the joint-guidance tests (tests/test_joint_guidance_cpu.py, tests/test_joint_guidance_gpu.py).  Nothing
here is taken from the code under test.

(a) ``combine64``: eps = e + (s_c - 1)(e - n_c) + (s_l - 1)(e - n_l) in float64 (include/srgd_hip.h, srgd_sampler_step with passes = 3).
(b) ``joint_tiled_sample``: ``oracle.srgd_oracle.tiled_sample``'s loop restated from the oracle's own functions, as
    tests/guidance_cases.py does.  A step on which both scales are current goes through ``joint_predict_and_step``: three calls of
    ``oracle.unet_forward`` combined by (a), then ``O.predict_and_step``'s own step lines; every other step goes through
    ``O.predict_and_step`` itself.  With one scale at 1 the loop is the oracle's bit for bit (asserted on the CPU).
``MUTANTS`` are three deliberate errors of (b)'s joint step; ``step64`` is the DDPM step in float64 on fp32 step scalars, what the
one-step GPU test applies to the product's own three U-Net evaluations.

Geometry.  An image that fits a tile has a canvas of one tile (``get_coord_and_pad``): the 256 x 256 image of the end-to-end case is
one tile in both grids.  Where more than one tile, more than one launch or a partial last launch matters the tests use the
300 x 300 image as well: a 768 x 768 canvas, 9 even and 4 odd tiles.

The x_start bar of the one-step GPU test (4 x the larger of the parent's two two-pass deviations, measured in that test) is not known
on the CPU.  That test asserts that its bar stays below ``ONE_STEP_BAR_CAP``, the project's own bar on x_start trajectories, and
the CPU sensitivity test shows that every mutant moves x_start by more than ``MUTANT_FACTOR`` x that cap: a fortiori by more than
100 x the bar the GPU test uses."""
import functools
import json
import os

import torch
import torch.nn.functional as F

from oracle import srgd_oracle as O
from srgd_amd.synth import synth_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 16
LABEL = 1
S_C, S_L = 1.5, 2.0                     # the end-to-end case
SENS_S_C, SENS_S_L = 1.5, 3.0           # the one-step and sensitivity case: unequal on purpose
WEIGHT_SEED = 0                         # synth_state_dict seed of every random-weight test here (the sensitivity holds for it)
FINAL_BAR, TRAJECTORY_BAR = 1e-3, 2e-3  # the project's bars of an fp32 / f16x3 run against the oracle on the same noise
ONE_STEP_BAR_CAP = TRAJECTORY_BAR
MUTANT_FACTOR = 100.0
MUTANTS = ("scales_swapped", "pass1_keeps_condition", "pass2_on_label_row")
ONE_STEP_INDEX, ONE_STEP_STEPS = 40, 50  # the one-step test: even grid, alpha = 0.82; 57 % of the predicted x0 are off the clamp

E2E = dict(size=(256, 256), steps=4, cond_scale=S_C, class_cond_scale=S_L, class_guidance_start_steps=1, guidance_start_steps=2,
           batch_size=4, seed=83)


def combine64(e, n_c, n_l, s_c, s_l):
    """(a): the definition, in float64."""
    e, n_c, n_l = e.double(), n_c.double(), n_l.double()
    return e + (float(s_c) - 1.0) * (e - n_c) + (float(s_l) - 1.0) * (e - n_l)


def cond_guided64(e, n_c, s_c):
    """model.py:3150 in float64."""
    return n_c.double() + (e.double() - n_c.double()) * float(s_c)


def class_guided64(e, n_l, s_l):
    """model.py:3154 in float64."""
    return n_l.double() + (e.double() - n_l.double()) * float(s_l)


def step64(x, eps64, z, sc, last=False):
    """x0 and the canvas after the step (model.py:3160-3164, :3187-3188) in float64; ``sc``: the run's fp32 step scalars as a dict of
    Python floats (alpha, sigma, alpha_next, c, one_minus_c, noise_scale)."""
    x = x.double()
    x0 = ((x - sc["sigma"] * eps64) / sc["alpha"]).clamp(-1.0, 1.0)
    mean = sc["alpha_next"] * (x * sc["one_minus_c"] / sc["alpha"] + sc["c"] * x0)
    if not last:
        mean = mean + sc["noise_scale"] * z.double()
    return mean, x0


def joint_predict_and_step(sd, cfg, x, t, t_next, cond, class_label, s_c, s_l, noise, trace=None, mutant=None, unet=None):
    """``O.predict_and_step`` for a joint step: three U-Net evaluations, (a), then its own lines.  ``unet``: as the oracle's, a
    replacement for ``O.unet_forward`` (the sensitivity test memoises it: the mutants repeat evaluations)."""
    assert mutant is None or mutant in MUTANTS
    unet = unet or O.unet_forward
    s = O.step_scalars(t, t_next)
    ls = s["log_snr"].expand(x.shape[0])
    e = unet(sd, cfg, x, ls, class_label, cond)
    n_c = unet(sd, cfg, x, ls, class_label, cond if mutant == "pass1_keeps_condition" else None)
    n_l = unet(sd, cfg, x, ls, class_label if mutant == "pass2_on_label_row" else None, cond)
    if mutant == "scales_swapped":
        s_c, s_l = s_l, s_c
    eps = combine64(e, n_c, n_l, s_c, s_l).to(x.dtype)
    x0 = ((x - s["sigma"] * eps) / s["alpha"]).clamp(-1.0, 1.0)
    mean = s["alpha_next"] * (x * (1 - s["c"]) / s["alpha"] + s["c"] * x0)
    if trace is not None:
        trace.setdefault("eps", []).append(eps.clone())
    if t_next == 0:
        return mean, x0
    z = noise.randn(x.shape).to(x.dtype)
    return mean + s["var"].sqrt() * z, x0


def joint_tiled_sample(sd, cfg, condition_x, class_label=None, *, batch_size=4, num_sample_steps=50, cond_scale=1.0,
                       guidance_start_steps=0, class_cond_scale=1.0, class_guidance_start_steps=0, tile=256, noise=None, trace=None,
                       mutant=None):
    """(b): ``O.tiled_sample`` from white noise with the joint step where both scales are current."""
    noise = noise or O.NoiseSource()
    cond = condition_x * 2 - 1
    _, _, h, w = cond.shape
    (left, top, right, bottom), pad = O.canvas_box_and_pad(h, w)
    cond = F.pad(cond, pad, mode="reflect")
    img = noise.randn(cond.shape)
    steps = torch.linspace(1.0, 0.0, num_sample_steps + 1)
    hp, wp = cond.shape[-2:]
    grids = O.sampling_grids(hp, wp, tile, tile)
    (il, it, ir, ib), ipad = O.grid_bbox(grids[1], hp, wp)
    cond = F.pad(cond[:, :, it:ib, il:ir], ipad, mode="constant", value=0.0)
    x_start = img.clone()
    for i in range(num_sample_steps):
        cs = cond_scale if i >= guidance_start_steps else 1.0
        ccs = class_cond_scale if i >= class_guidance_start_steps else 1.0
        t, t_next = steps[i], steps[i + 1]
        boxes = grids[i % 2]
        for j in range(0, len(boxes), batch_size):
            chunk = boxes[j:j + batch_size]
            xb = torch.cat([img[:, :, a:b, c:d] for (a, b, c, d) in chunk], dim=0)
            cb = torch.cat([cond[:, :, a:b, c:d] for (a, b, c, d) in chunk], dim=0)
            if cs != 1.0 and ccs != 1.0:
                out, x0 = joint_predict_and_step(sd, cfg, xb, t, t_next, cb, class_label, cs, ccs, noise, None, mutant)
            else:
                out, x0 = O.predict_and_step(sd, cfg, xb, t, t_next, cb, class_label, cs, ccs, noise, None)
            for k, (a, b, c, d) in enumerate(chunk):
                img[:, :, a:b, c:d] = out[k]
                x_start[:, :, a:b, c:d] = x0[k]
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


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def state_dict(weight_seed=WEIGHT_SEED):
    with open(os.path.join(ROOT, "tests", "golden", f"schema_dim{DIM}.json")) as f:
        schema = {k: tuple(v) for k, v in json.load(f).items()}
    return synth_state_dict(schema, seed=weight_seed)


def condition(h, w, k=0):
    """A condition [1,3,h,w] in [0,1]: smooth with texture (a plain random one makes e - n_c all noise)."""
    g = torch.Generator().manual_seed(900 + k)
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    base = torch.stack([0.5 + 0.35 * torch.sin(x / 17.0 + k) * torch.cos(y / 23.0), 0.2 + 0.6 * x / w, 0.5 + 0.3 * torch.cos((x + y) / 29.0)])
    return (base + 0.08 * (torch.rand(3, h, w, generator=g) - 0.5)).clamp(0.0, 1.0)[None]


def label():
    return torch.tensor([LABEL])


def with_seed(seed, fn):
    """``fn()`` after ``torch.manual_seed(seed)``; the caller's generator is restored."""
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    try:
        with torch.inference_mode():
            return fn()
    finally:
        torch.set_rng_state(state)


@functools.lru_cache(maxsize=None)
def e2e_oracle():
    """(output [1,3,H,W], {"img": [...], "x_start": [...]}) of (b) on the end-to-end case; made once, shared, read-only."""
    trace = {}
    kw = {k: E2E[k] for k in ("batch_size", "cond_scale", "class_cond_scale", "class_guidance_start_steps", "guidance_start_steps")}
    out = with_seed(E2E["seed"], lambda: joint_tiled_sample(O.strip_model_prefix(state_dict()), O.UnetCfg(dim=DIM), condition(*E2E["size"]),
                                                             label(), num_sample_steps=E2E["steps"], trace=trace, **kw))
    return out, trace


@functools.lru_cache(maxsize=None)
def one_step_inputs(h, w):
    """(canvas before the step [1,3,hp,wp], condition [1,3,h,w], tile noise of the even grid [n,3,256,256]) of the one-step test."""
    (_, _, _, _), pad = O.canvas_box_and_pad(h, w)
    hp, wp = h + pad[2] + pad[3], w + pad[0] + pad[1]
    g = torch.Generator().manual_seed(4242)
    n = len(O.sampling_grids(hp, wp)[0])
    return torch.randn(1, 3, hp, wp, generator=g), condition(h, w, 1), torch.randn(n, 3, 256, 256, generator=g)


# ------------------------------------------------------------------------------------------------ the closed-form network
# tests/sampler_cases.py's designed network ignores the label: e == n_l, the third term of (a) is exactly zero and a joint run with
# (s_c, s_l) is the condition-guided run with s_c, whatever s_l - unless pass 2 lost the condition or pass 1 kept it.  Two steps:
# one on the even grid, one on the odd grid with its ring.  The references, distances and tolerances are that module's own
# construction (``sampler_cases.tolerances``) applied to these two cases.
def _closed_form_cases():
    from tests import sampler_cases as S
    return {"img256": S._case("joint_img256", "ddpm_tiled", 256, 256, 40, 31, 2, batch_size=4, cond_scale=SENS_S_C),
            "img300": S._case("joint_img300", "ddpm_tiled", 300, 300, 41, 32, 2, batch_size=4, cond_scale=SENS_S_C)}


@functools.lru_cache(maxsize=None)
def closed_form_case(key):
    return _closed_form_cases()[key]


@functools.lru_cache(maxsize=None)
def closed_form_reference(key):
    """(tensors, trace) of the float64 condition-guided oracle run on the closed form; shared, read-only."""
    from tests import sampler_cases as S
    return S.reference_run(closed_form_case(key))


@functools.lru_cache(maxsize=None)
def closed_form_tolerances(key, precision):
    """``sampler_cases.tolerances`` for these cases: 8 x E32 (+ 8 x E_split for f16x3), floored at 4 ulp."""
    from tests import sampler_cases as S
    assert precision in ("fp32", "f16x3")
    case = closed_form_case(key)
    ref, _ = closed_form_reference(key)
    e32 = S.distances(S.reference_run(case, torch.float32)[0], ref)
    esp = S.distances(S.reference_run(case, torch.float64, round_inputs=S.split_round)[0], ref)
    return {k: max(S.MARGIN * e32[k] + (S.MARGIN * esp[k] if precision == "f16x3" else 0.0), S.floor_of(ref[k])) for k in ref}
