"""Closed-form float64 references for the sampler step kernels (srgd_amd/csrc/sampler.hip).  CPU only; shared by
tests/test_sampler_cases_cpu.py (which checks the construction, derives every tolerance and shows that the assertions reject wrong
samplers) and tests/test_sampler_exact_gpu.py (which holds the kernels to those tolerances).

The network is taken out of the comparison by DESIGNED weights (``pointwise_state_dict``): with the last ResnetBlock's second
GroupNorm zeroed, the trunk's half of its ``res_conv`` zeroed and ``init_conv`` reduced to its centre tap, the whole U-Net is

    eps(p) = M [x(p); cond(p)] + b,        M = F R A   (final_conv, kept half of res_conv, centre tap of init_conv)

while every production kernel still runs on random weights and contributes 0 x finite = 0.  A and R are selections with
power-of-two gains and F, b are short dyadic numbers, so in bf16 mode every activation after ``init_gather_kernel``'s rounding of
[x; cond] is an exact bf16 value: ``pointwise_eps(..., round_inputs=torch.bfloat16)`` is the complete model of that mode.

References.  Whole runs: the oracle's samplers with ``unet=`` the closed form, in float64 on the fp32 noise of the run.  One step:
``ddpm_step`` / ``edm_heun_step`` / ``edm_dpmpp_step`` on canvases (a step touches every pixel of its grid exactly once, so on the
canvas it is a pointwise map); ``canvas_run`` chains them with the traced noise and is the oracle's run again (asserted on the
CPU) - it is what the mutants mutate.

Tolerances (``tolerances``): per compared tensor, fp32 = 8 x E32 with E32 the distance of the fp32 oracle run from the float64 one
on the same noise, floored at 4 ulp of the tensor's largest magnitude; f16x3 adds 8 x E_split, the distance from exact of the
float64 run whose eps goes through oracle/split_emulation.py's operand split; device noise adds 32 x the distance the Philox
restatement's own float32 evaluation moves the float64 run (the factor tests/test_device_noise_gpu.py grants the device's fast
intrinsics).  Nothing here is taken from the code under test.
"""
from __future__ import annotations

import functools
import json
import math
import os
from typing import Dict

import numpy as np
import torch

from oracle import philox as P
from oracle import split_emulation as SE
from oracle import srgd_oracle as O
from srgd_amd.synth import synth_state_dict

G = os.path.join(os.path.dirname(__file__), "golden")
TILE = 256
MARGIN = 8                  # FMA contraction, a reciprocal for a division, another summation order over C: a few ulp each
FLOOR_ULPS = 4
DEVICE_NOISE_MARGIN = 32    # tests/test_device_noise_gpu.py: the device's draws lie within 32 x the float32 floor of the restatement
MUTANT_FACTOR = 100.0
SATURATION_CAP = 0.25
DEVICE_SEED = 71


def schema(dim: int, prefix: str = "model.") -> Dict[str, tuple]:
    with open(os.path.join(G, f"schema_dim{dim}.json")) as f:
        return {prefix + k[len("model."):]: tuple(v) for k, v in json.load(f).items()}


# ------------------------------------------------------------------------------------------------ the designed network
DDPM_SPEC = dict(diag=2.0, bias_den=16, bias_max=2)
EDM_SPEC = dict(diag=-2.0, bias_den=16, bias_max=2)


def pointwise_state_dict(schema_: Dict[str, tuple], spec: dict, seed: int = 0) -> Dict[str, torch.Tensor]:
    """``synth_state_dict(schema_, seed)`` with the three designed changes.  Hidden channel j of ``init_conv`` carries input plane
    j % 6 times 2^ka_j (centre tap only, bias 0); ``final_res_block.res_conv`` passes channel j of r on times 2^kr_j (trunk half
    and bias 0); ``final_conv`` is m / 16 * 2^-s with m = 8 where channel j carries the output's own x plane and m = +-1, +-2
    elsewhere, so M = [D + mixing | mixing] with a diagonal D of the sign of ``spec["diag"]`` - positive for DDPM (an eps that
    grows with x keeps the predicted x0 off the clamp), negative for EDM (c_skip x + c_out F wants F = -x to contract) -; its bias
    is m / bias_den with |m| <= bias_max; 2^-s brings the largest |entry| of D to at most ``|spec["diag"]|``."""
    sd = dict(synth_state_dict(schema_, seed=seed))
    pre = next(k for k in schema_ if k.endswith("init_conv.weight"))[:-len("init_conv.weight")]
    g = torch.Generator().manual_seed(1000 + seed)
    dim = schema_[pre + "init_conv.weight"][0]
    assert schema_[pre + "init_conv.weight"] == (dim, 6, 7, 7) and schema_[pre + "final_conv.weight"] == (3, dim, 1, 1)
    assert schema_[pre + "final_res_block.res_conv.weight"] == (dim, 2 * dim, 1, 1)
    ka = torch.randint(-1, 2, (dim,), generator=g)
    kr = torch.randint(-1, 2, (dim,), generator=g)
    a = torch.zeros(dim, 6, 7, 7)
    r = torch.zeros(dim, 2 * dim, 1, 1)
    for j in range(dim):
        a[j, j % 6, 3, 3] = 2.0 ** int(ka[j])
        r[j, dim + j, 0, 0] = 2.0 ** int(kr[j])
    m = torch.randint(1, 3, (3, dim), generator=g) * (torch.randint(0, 2, (3, dim), generator=g) * 2 - 1)
    sign = 1 if spec["diag"] > 0 else -1
    for j in range(dim):
        if j % 6 < 3:
            m[j % 6, j] = 8 * sign
    f = m.double() / 16.0
    gain = 2.0 ** (ka + kr).double()
    diag = max(sum(float(f[o, j] * gain[j]) for j in range(o, dim, 6)) * sign for o in range(3))
    shift = max(0, math.ceil(math.log2(diag / abs(spec["diag"]))))
    assert shift <= 8                                            # m / 16 * 2^-s stays a normal f16 number
    f = f * 2.0 ** -shift
    bias = torch.randint(-spec["bias_max"], spec["bias_max"] + 1, (3,), generator=g).double() / spec["bias_den"]
    for leaf in ("weight", "bias"):
        sd[pre + "final_res_block.block2.norm." + leaf] = torch.zeros(dim)
    sd[pre + "init_conv.weight"], sd[pre + "init_conv.bias"] = a, torch.zeros(dim)
    sd[pre + "final_res_block.res_conv.weight"], sd[pre + "final_res_block.res_conv.bias"] = r, torch.zeros(dim)
    sd[pre + "final_conv.weight"], sd[pre + "final_conv.bias"] = f.float().reshape(3, dim, 1, 1), bias.float()
    assert set(sd) == set(schema_) and all(tuple(sd[k].shape) == tuple(schema_[k]) for k in sd)
    return sd


def closed_form_of(sd: Dict[str, torch.Tensor]):
    """(M [3,6], b [3]) in float64, read off the state dict itself: M = F R A."""
    pre = next(k for k in sd if k.endswith("init_conv.weight"))[:-len("init_conv.weight")]
    dim = sd[pre + "init_conv.weight"].shape[0]
    a = sd[pre + "init_conv.weight"][:, :, 3, 3].double()
    r = sd[pre + "final_res_block.res_conv.weight"][:, dim:, 0, 0].double()
    f = sd[pre + "final_conv.weight"][:, :, 0, 0].double()
    return f @ r @ a, sd[pre + "final_conv.bias"].double()


def split_round(v: torch.Tensor) -> torch.Tensor:
    """The value the f16x3 kernels see of an fp32 operand: its two f16 halves (oracle/split_emulation.py), summed exactly."""
    hi, lo = SE.halves(v.float(), "f16")
    return hi.double() + lo.double()


def pointwise_eps(M, b, x, cond, dtype, round_inputs=None):
    """eps = M [x; cond] + b in ``dtype``.  ``round_inputs``: None, a dtype ([x; cond] rounded to it from fp32:
    ``torch.bfloat16`` is the model of the bf16 mode) or a callable on the fp32-valued planes."""
    if round_inputs is None:
        rnd = lambda v: v
    elif callable(round_inputs):
        rnd = round_inputs
    else:
        rnd = lambda v: v.float().to(round_inputs)
    M, b = M.to(dtype), b.to(dtype)
    e = torch.einsum("oi,bihw->bohw", M[:, :3], rnd(x).to(dtype))
    if cond is not None:
        e = e + torch.einsum("oi,bihw->bohw", M[:, 3:], rnd(cond).to(dtype))
    return e + b.view(1, 3, 1, 1)


def closed_unet(M, b, round_inputs=None):
    """The ``unet=`` callable of the oracle's samplers."""
    return lambda sd, cfg, x, log_snr, class_label, cond: pointwise_eps(M, b, x, cond, x.dtype, round_inputs)


@functools.lru_cache(maxsize=None)
def designed(dim: int, kind: str = "ddpm"):
    """(state dict with the wrapper's key prefix, M, b) of the designed network for the DDPM or the EDM wrapper."""
    sd = pointwise_state_dict(schema(dim, "model." if kind == "ddpm" else "net."), DDPM_SPEC if kind == "ddpm" else EDM_SPEC, 0)
    return (sd,) + closed_form_of(sd)


# ------------------------------------------------------------------------------------------------ one-step references
def ddpm_step(M, b, x, cond, z, s, *, scale=1.0, guided=False, last=False, round_inputs=None, mutant=None, x_null=None):
    """One DDPM step (model.py:3147-3188) on equally shaped [B,3,h,w] pieces of the canvas before the step, the condition canvas
    and the step's noise canvas; ``s``: ``O.step_scalars`` of the step (fp32 values).  ``guided``: LR-condition guidance with
    ``scale`` (two passes).  Returns (canvas after the step, x_start) in x's dtype."""
    dt = x.dtype
    e = pointwise_eps(M, b, x, cond, dt, round_inputs)
    if guided:
        n = pointwise_eps(M, b, x if x_null is None else x_null, None, dt, round_inputs)
        if mutant == "passes_swapped":
            e, n = n, e
        e = n + (e - n) * scale
    x0 = (x - s["sigma"] * e) / s["alpha"]
    x0c = x0.clamp(-1.0, 1.0)
    c = s["c"]
    w_x0 = (1 - c) if mutant == "one_minus_c_for_c" else c
    mean = s["alpha_next"] * (x * (1 - c) / s["alpha"] + w_x0 * x0c)
    if not last or mutant == "noise_on_last":
        mean = mean + s["var"].sqrt() * z
    return mean, (x0 if mutant == "x_start_unclamped" else x0c)


def edm_scalars(e: O.EdmCfg, n: int, i: int) -> dict:
    """The fp32 values of EDM step i of an n-step run (model.py:2333-2337, :2388, preconditioning of both passes), as Python
    floats; what the oracle's loop uses and what the wrappers hand the kernels."""
    sig = O.edm_sigmas(e, n)
    gam = O.edm_gammas(e, sig, n)
    sigma, sigma_next, gamma = sig[i].item(), sig[i + 1].item(), gam[i].item()
    sigma_hat = sigma + gamma * sigma
    out = dict(s_noise=O._f32(e.S_noise), hat_coef=O._f32(math.sqrt(sigma_hat ** 2 - sigma ** 2)), sigma_hat=O._f32(sigma_hat),
               sigma_next=sigma_next, dt=O._f32(sigma_next - sigma_hat), half_dt=O._f32(0.5 * (sigma_next - sigma_hat)))
    for tag, v in (("hat", sigma_hat), ("next", sigma_next)):
        c = O.edm_precond_coeffs(e, torch.full((1,), v))
        for k in ("c_in", "c_skip", "c_out"):
            out[f"{k}_{tag}"] = float(c[k])
    return out


def _edm_denoise(M, b, x, cond, c_in, c_skip, c_out, scale, guided, clamp, round_inputs):
    xin = c_in * x
    net = pointwise_eps(M, b, xin, cond, x.dtype, round_inputs)
    out = c_skip * x + c_out * net
    if guided:
        null = c_skip * x + c_out * pointwise_eps(M, b, xin, None, x.dtype, round_inputs)
        out = null + (out - null) * scale
    return out.clamp(-1.0, 1.0) if clamp else out


def edm_heun_step(M, b, x, cond, z, sc, *, scale=1.0, guided=False, clamp=True, round_inputs=None, mutant=None):
    """One stochastic Heun step (model.py:2386-2414) on pieces of the canvases; ``z``: the unit noise canvas; ``sc``:
    ``edm_scalars``.  Returns (canvas after the step, the slope the reference keeps as x_start)."""
    s_noise = 1.0 if mutant == "s_noise_dropped" else sc["s_noise"]
    xh = x + sc["hat_coef"] * (s_noise * z)
    den = _edm_denoise(M, b, xh, cond, sc["c_in_hat"], sc["c_skip_hat"], sc["c_out_hat"], scale, guided, clamp, round_inputs)
    d = (xh - den) / sc["sigma_hat"]
    nxt = xh + sc["dt"] * d
    if sc["sigma_next"] == 0 and mutant != "last_step_heun":
        return nxt, d
    x2 = nxt + sc["hat_coef"] * (s_noise * z) if mutant == "hat_coef_both_passes" else nxt
    c_skip2 = sc["c_skip_hat"] if mutant == "c_skip_hat_second_pass" else sc["c_skip_next"]
    den2 = _edm_denoise(M, b, x2, cond, sc["c_in_next"], c_skip2, sc["c_out_next"], scale, guided, clamp, round_inputs)
    d2 = (x2 - den2) / sc["sigma_next"]
    return xh + sc["half_dt"] * (d + d2), d2


def dpmpp_scalars(e: O.EdmCfg, n: int, i: int, first: int) -> dict:
    """Step i of sample_using_dpmpp (model.py:2513-2541) in the reference's fp32 tensor ops; ``first``: the first executed step."""
    sig = O.edm_sigmas(e, n)
    t_of = lambda s: s.log().neg()
    t, t_next = t_of(sig[i]), t_of(sig[i + 1])
    h = t_next - t
    gamma = None
    if i != first and sig[i + 1] != 0:
        gamma = -1 / (2 * ((t - t_of(sig[i - 1])) / h))
    c = O.edm_precond_coeffs(e, torch.full((1,), sig[i].item()))
    return dict(ratio=t_next.neg().exp() / t.neg().exp(), em1=(-h).expm1(), gamma=gamma, c_in=float(c["c_in"]),
                c_skip=float(c["c_skip"]), c_out=float(c["c_out"]))


def edm_dpmpp_step(M, b, x, cond, old, sc, *, scale=1.0, guided=False, clamp=True, round_inputs=None, mutant=None):
    """Returns (canvas after the step, the extrapolated denoised image kept as x_start, the denoised image = next ``old``)."""
    den = _edm_denoise(M, b, x, cond, sc["c_in"], sc["c_skip"], sc["c_out"], scale, guided, clamp, round_inputs)
    g = None if mutant == "dpm_history_dropped" else sc["gamma"]
    den_d = den if g is None else (1 - g) * den + g * old
    return sc["ratio"] * x - sc["em1"] * den_d, den_d, den


# ------------------------------------------------------------------------------------------------ cases
def _rand_cond(h, w, k, b=1):
    return torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(500 + k))


def _case(name, kind, h, w, k, seed, steps, b=1, device_noise=False, dim=16, **kw):
    return dict(name=name, kind=kind, h=h, w=w, k=k, seed=seed, steps=steps, b=b, device_noise=device_noise, dim=dim, kw=kw)


# conditions: 64 x 64 -> 256^2 (one tile), 75 x 75 -> 300^2 (768^2 canvas, 9 / 4 tiles, shifted grid), 75 x 125 -> 300 x 500 (12 / 6)
CASES = [
    _case("ddpm_plain", "ddpm_tiled", 300, 300, 0, 11, 4, batch_size=4),                      # 9 / 4 tiles in minibatches of 4
    _case("ddpm_cfg", "ddpm_tiled", 300, 500, 1, 12, 4, batch_size=5, cond_scale=2.0, guidance_start_steps=2),
    _case("ddpm_late_start", "ddpm_tiled", 256, 256, 2, 13, 4, batch_size=4, generation_start_steps=2),
    _case("ddpm_no_white", "ddpm_tiled", 256, 256, 3, 14, 3, batch_size=4, start_white_noise=False),
    _case("ddpm_device_noise", "ddpm_tiled", 256, 256, 4, DEVICE_SEED, 4, device_noise=True, batch_size=4),
    # the images of the groups, each as its own run: a mixed-size list with seeds [3, 4], a [2,3,300,300] batch on one stream
    _case("ddpm_group_a", "ddpm_tiled", 300, 300, 5, 3, 3, batch_size=4),
    _case("ddpm_group_b", "ddpm_tiled", 256, 512, 6, 4, 3, batch_size=4),
    _case("ddpm_batch_0", "ddpm_tiled", 300, 300, 7, 5, 3, batch_size=4),
    _case("ddpm_batch_1", "ddpm_tiled", 300, 300, 8, 5, 3, batch_size=4),
    _case("ddpm_dim128", "ddpm_tiled", 256, 256, 9, 15, 2, dim=128, batch_size=4),
    _case("edm_plain", "edm_tiled", 300, 300, 10, 21, 4, batch_size=4),
    _case("edm_no_clamp", "edm_tiled", 256, 256, 11, 22, 4, batch_size=4, clamp=False),
    _case("edm_cfg", "edm_tiled", 300, 500, 12, 23, 4, batch_size=5, cond_scale=1.5, guidance_start_steps=2),
    _case("edm_late_start", "edm_tiled", 256, 256, 13, 24, 6, batch_size=4, generation_start_steps=3),
    _case("edm_zero_init", "edm_tiled", 256, 256, 14, 25, 4, batch_size=4, zero_init=True),
    _case("edm_sample_b2", "edm_sample", 256, 256, 15, 26, 4, b=2),
    _case("edm_dpmpp_b1", "edm_dpmpp", 256, 256, 16, 27, 5, b=1),
    _case("edm_dpmpp_b2", "edm_dpmpp", 256, 256, 17, 28, 5, b=2),
]
CASE = {c["name"]: c for c in CASES}
EDM = O.EdmCfg()                                  # the defaults: churn is active (S_churn 80); constructor schedule of 32 steps


def condition(case) -> torch.Tensor:
    return _rand_cond(case["h"], case["w"], case["k"], case["b"])


def one_tile_device_plan(seed: int, n: int, first: int = 0, dtype=np.float64):
    """``P.device_noise_draws("ddpm_tiled", ...)`` of a one-tile image (asserted equal on the CPU), with the restatement evaluated in
    ``dtype``: np.float32 is its rounding-floor twin."""
    t = lambda z, *shape: torch.from_numpy(np.asarray(z).astype(np.float32)).reshape(*shape)
    nel = 3 * TILE * TILE
    draws = [t(P.philox_normal(nel, seed, P.STREAM_START, None, dtype), 1, 3, TILE, TILE)]
    for i in range(first, n):
        if i != n - 1:
            draws.append(t(P.philox_normal(nel, seed, P.STREAM_TILES, i, dtype), 1, 3, TILE, TILE))
        if i % 2 == 1:
            draws.append(t(P.philox_normal(nel, seed, P.STREAM_RING, i, dtype), 1, 3, TILE, TILE))
    return draws


def _noise_of(case, twin=False):
    if not case["device_noise"]:
        torch.manual_seed(case["seed"])
        return O.NoiseSource()
    assert case["h"] == case["w"] == TILE
    return O.ReplayNoise(one_tile_device_plan(case["seed"], case["steps"], case["kw"].get("generation_start_steps", 0),
                                              np.float32 if twin else np.float64))


def geometry(case):
    """(crop box (top, bottom, left, right), inner box likewise, canvas (hp, wp)) of a tiled case."""
    h, w = case["h"], case["w"]
    (left, top, right, bottom), pad = O.canvas_box_and_pad(h, w)
    hp, wp = h + pad[2] + pad[3], w + pad[0] + pad[1]
    (il, it, ir, ib), _ = O.grid_bbox(O.sampling_grids(hp, wp, TILE, TILE)[1], hp, wp)
    return (top, bottom, left, right), (it, ib, il, ir), (hp, wp)


def reference_run(case, dtype=torch.float64, round_inputs=None, twin_noise=False):
    """The oracle's run of a case on the closed form.  Returns (tensors, trace): ``tensors`` is the ordered dict of what a GPU
    run is compared on - "img0" (the start inside the crop box), "img{k}" / "x0_{k}" (canvases after the k-th executed step),
    "final" ([0,1]) - and ``trace`` the oracle's."""
    _, M, b = designed(case["dim"], "ddpm" if case["kind"] == "ddpm_tiled" else "edm")
    unet = closed_unet(M, b, round_inputs)
    cond = condition(case).to(dtype)
    noise = _noise_of(case, twin_noise)
    trace = {}
    cfg = O.UnetCfg(dim=case["dim"])
    with torch.inference_mode():
        if case["kind"] == "ddpm_tiled":
            final = O.tiled_sample({}, cfg, cond, None, num_sample_steps=case["steps"], noise=noise, trace=trace, unet=unet,
                                   **case["kw"])
        elif case["kind"] == "edm_tiled":
            final = O.edm_tiled_sample({}, cfg, EDM, cond, None, num_sample_steps=case["steps"], noise=noise, trace=trace,
                                       unet=unet, **case["kw"])
        elif case["kind"] == "edm_sample":
            final = O.edm_sample({}, cfg, EDM, cond, None, num_sample_steps=case["steps"], noise=noise, trace=trace, unet=unet,
                                 **case["kw"])
        else:
            final = O.edm_sample_dpmpp({}, cfg, EDM, cond, None, num_sample_steps=case["steps"], noise=noise, trace=trace,
                                       unet=unet, **case["kw"])
    if case["device_noise"]:
        assert noise.i == len(noise.draws), "the run must consume the whole draw plan"
    return pack(case, trace["start"], trace["img"], trace["x_start"], final), trace


def pack(case, start, imgs, x0s, final):
    out = {}
    if case["kind"].endswith("_tiled"):
        (top, bottom, left, right), _, _ = geometry(case)
        start = start[:, :, top:bottom, left:right]
    out["img0"] = start
    for k, (a, x0) in enumerate(zip(imgs, x0s)):
        out[f"img{k + 1}"], out[f"x0_{k + 1}"] = a, x0
    out["final"] = final
    return out


def executed_steps(case):
    return list(range(case["kw"].get("generation_start_steps", 0), case["steps"]))


def _guided(case, i):
    cs = case["kw"].get("cond_scale", 1.0)
    return cs != 1.0 and i >= case["kw"].get("guidance_start_steps", 0), cs


def canvas_run(case, trace, dtype=torch.float64, round_inputs=None, mutant=None):
    """The run again, from the one-step references on whole canvases and the traced noise.  Unmutated it is the oracle's run (the
    CPU suite asserts so); ``mutant`` names one deliberate error of the recurrence."""
    _, M, b = designed(case["dim"], "ddpm" if case["kind"] == "ddpm_tiled" else "edm")
    kw, n = case["kw"], case["steps"]
    img = trace["start"].to(dtype).clone()
    start = img.clone()
    cond = trace["cond"].to(dtype) if "cond" in trace else condition(case).to(dtype) * 2 - 1
    tiled = case["kind"].endswith("_tiled")
    if tiled:
        _, (it, ib, il, ir), _ = geometry(case)
    else:
        it, ib, il, ir = 0, img.shape[-2], 0, img.shape[-1]
    x_start = img.clone()
    imgs, x0s = [], []
    old = None
    ts = torch.linspace(1.0, 0.0, n + 1)
    roll = lambda v: torch.roll(v, TILE, dims=-1)
    for k, i in enumerate(executed_steps(case)):
        whole = i % 2 == 0 or not tiled or mutant == "parity_not_alternated"
        box = (slice(None), slice(None)) + ((slice(None), slice(None)) if whole else (slice(it, ib), slice(il, ir)))
        guided, scale = _guided(case, i)
        x, cnd = img[box], cond[box]
        if case["kind"] == "ddpm_tiled":
            z = trace["noise"][k]
            last = i == n - 1
            if mutant == "noise_on_last" and last:
                z = trace["noise"][k - 1]
            z = z.to(dtype)
            if mutant == "noise_tile_off_by_one":
                z = roll(z)
            x_null = roll(img)[box] if mutant == "second_pass_one_tile_late" else None
            new, x0 = ddpm_step(M, b, x, cnd, z[box], O.step_scalars(ts[i], ts[i + 1]), scale=scale, guided=guided, last=last,
                                round_inputs=round_inputs, mutant=mutant, x_null=x_null)
        elif case["kind"] in ("edm_tiled", "edm_sample"):
            new, x0 = edm_heun_step(M, b, x, cnd, trace["noise"][k].to(dtype)[box], edm_scalars(EDM, n, i), scale=scale,
                                    guided=guided, clamp=kw.get("clamp", True), round_inputs=round_inputs, mutant=mutant)
        else:
            new, x0, old = edm_dpmpp_step(M, b, x, cnd, old, dpmpp_scalars(EDM, n, i, executed_steps(case)[0]), scale=scale,
                                          guided=guided, clamp=kw.get("clamp", True), round_inputs=round_inputs, mutant=mutant)
        img[box], x_start[box] = new, x0
        ring = trace["ring"][k] if tiled else None
        if ring is not None and mutant != "ring_renoise_skipped":
            sigma = (-O.log_snr_linear(ts[i + 1])).sigmoid().sqrt() if case["kind"] == "ddpm_tiled" \
                else O.edm_sigmas(EDM, EDM.num_sample_steps)[i]
            inner = img[:, :, it:ib, il:ir].clone()
            img = ring.to(dtype) * sigma
            img[:, :, it:ib, il:ir] = inner
        imgs.append(img.clone())
        x0s.append(x_start.clone())
    if tiled:
        (top, bottom, left, right), _, _ = geometry(case)
        final = img[:, :, top:bottom, left:right]
    else:
        final = img
    return pack(case, start, imgs, x0s, (final.clamp(-1.0, 1.0) + 1) * 0.5)


# ------------------------------------------------------------------------------------------------ distances and tolerances
def ulp32(v: float) -> float:
    """One float32 ulp at magnitude v."""
    return 2.0 ** (math.floor(math.log2(v)) - 23) if v > 0 else 2.0 ** -149


def distance(a: torch.Tensor, b: torch.Tensor) -> float:
    """max |a - b| in float64; infinite where either is not finite (a mutant may divide by zero)."""
    d = (a.double() - b.double()).abs()
    return float("inf") if not bool(torch.isfinite(d).all()) else float(d.max())


def distances(run: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor]) -> Dict[str, float]:
    assert list(run) == list(ref), (list(run), list(ref))
    return {k: distance(run[k], ref[k]) for k in ref}


def floor_of(ref: torch.Tensor) -> float:
    return FLOOR_ULPS * ulp32(float(ref.abs().max()))


@functools.lru_cache(maxsize=None)
def _reference(name):
    return reference_run(CASE[name])


def reference(name):
    """(tensors, trace) of the float64 run of a case; computed once, shared, never written to."""
    return _reference(name)


@functools.lru_cache(maxsize=None)
def measured(name) -> Dict[str, Dict[str, float]]:
    """Per compared tensor: E32, E_split, E_noise (0 unless device noise) and the floor - from the oracle alone."""
    case = CASE[name]
    ref, _ = reference(name)
    e32 = distances(reference_run(case, torch.float32)[0], ref)
    esp = distances(reference_run(case, torch.float64, round_inputs=split_round)[0], ref)
    eno = distances(reference_run(case, torch.float64, twin_noise=True)[0], ref) if case["device_noise"] else {k: 0.0 for k in ref}
    return {k: dict(e32=e32[k], e_split=esp[k], e_noise=eno[k], floor=floor_of(ref[k])) for k in ref}


def tolerances(name, precision) -> Dict[str, float]:
    """The bound of every compared tensor of a case for a whole run in "fp32" or "f16x3"."""
    assert precision in ("fp32", "f16x3")
    out = {}
    for k, m in measured(name).items():
        t = MARGIN * m["e32"] + (MARGIN * m["e_split"] if precision == "f16x3" else 0.0) + DEVICE_NOISE_MARGIN * m["e_noise"]
        out[k] = max(t, m["floor"])
    return out


def one_step_tolerance(step32: torch.Tensor, step64: torch.Tensor, margin: float = MARGIN) -> float:
    """The bound of a one-step check: ``margin`` x the fp32-against-float64 distance of the SAME model on the same inputs."""
    return max(margin * distance(step32, step64), floor_of(step64))


def assert_run_within(run, ref, tol: Dict[str, float], report=None, **tags) -> Dict[str, float]:
    """Every compared tensor of ``run`` within its tolerance of ``ref``; the distances are reported before anything is asserted."""
    d = distances(run, ref)
    if report is not None:
        report(distances=d, tolerances=tol, **tags)
    bad = {k: (d[k], tol[k]) for k in d if not d[k] <= tol[k]}
    assert not bad, (tags, bad)
    return d


def assert_close(got: torch.Tensor, want: torch.Tensor, tol: float, what="") -> float:
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = distance(got, want)
    assert d <= tol, (what, d, tol)
    return d


def miss_factor(run, ref, tol: Dict[str, float]) -> float:
    """By how much the worst tensor of ``run`` misses its tolerance (> 1: the case fails)."""
    d = distances(run, ref)
    return max(d[k] / tol[k] for k in d)


def saturated_share(x: torch.Tensor, lo: float, hi: float) -> float:
    return float(((x <= lo) | (x >= hi)).double().mean())


# mutant -> the case that must reject it
MUTANTS = {
    "x_start_unclamped": "ddpm_plain",
    "passes_swapped": "ddpm_cfg",
    "second_pass_one_tile_late": "ddpm_cfg",
    "noise_on_last": "ddpm_plain",
    "noise_tile_off_by_one": "ddpm_plain",
    "parity_not_alternated": "ddpm_plain",
    "ring_renoise_skipped": "ddpm_plain",
    "one_minus_c_for_c": "ddpm_plain",
    "c_skip_hat_second_pass": "edm_plain",
    "s_noise_dropped": "edm_plain",
    "hat_coef_both_passes": "edm_plain",
    "last_step_heun": "edm_plain",
    "dpm_history_dropped": "edm_dpmpp_b2",
}
