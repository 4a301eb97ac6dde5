"""The sampler step kernels (srgd_amd/csrc/sampler.hip: init_gather, final_step, final_step_edm, the canvas kernels, and the eps4
hand-over of conv1x1_epilogue.hpp) against closed-form float64 references - tests/sampler_cases.py.

The samplers are the product's, loaded with the DESIGNED weights (the U-Net collapses to eps = M [x; cond] + b while every
production kernel still runs), so what is compared is the step arithmetic alone: guidance combine, x0 prediction and clamp,
posterior mean, per-tile noise lookup, ring re-noise, EDM preconditioning / churn / Heun / DPM-Solver++, crop and output map.

Whole runs (fp32, f16x3): every trajectory entry (``with_images``), every ``x_start`` entry (``with_x0_images``) and the final
image against the float64 run on the same noise.  Tolerance per tensor (``sampler_cases.tolerances``, computed from the oracle
alone): fp32 8 x E32, f16x3 8 x (E32 + E_split), floor 4 ulp of the tensor's largest magnitude.  bf16: the one-step check
(reference: the float64 step on bfloat16-rounded [x; cond] of the GPU's OWN previous canvas; tolerance 8 x the fp32-against-float64
distance of that same step) at every step, every pixel of the image.

Measured (E32, E_split, E_noise and the tolerances: on the CPU, from the oracle alone - tests/test_sampler_cases_cpu.py -s prints
every tensor; "GPU": the distance measured on an MI355X).  Per case the final image ([0,1]) and the tensor with the widest bound
(x0_1: 1 / alpha = 150 at t = 1; EDM's x0_k is the slope (x - D) / sigma, up to 1.8e3 at sigma_next = 0.002; the groups' list
form returns no trajectories).  The GPU's distance is about E32 everywhere, an eighth of the fp32 bound; final images were held to
1e-3 before.

    case               tensor  E32      E_split  E_noise  tol fp32 GPU fp32 tol f16x3 GPU f16x3
    ddpm_plain         final   1.2e-06  4.6e-07  0.0e+00  9.8e-06  5.1e-07  1.3e-05   5.1e-07
    ddpm_plain         x0_1    6.3e-05  4.8e-05  0.0e+00  5.1e-04  5.5e-05  8.9e-04   5.5e-05
    ddpm_cfg           final   1.1e-06  5.4e-07  0.0e+00  8.5e-06  6.0e-07  1.3e-05   6.0e-07
    ddpm_cfg           x0_1    7.4e-05  4.4e-05  0.0e+00  5.9e-04  6.4e-05  9.5e-04   6.4e-05
    ddpm_late_start    final   2.8e-07  2.4e-07  0.0e+00  2.2e-06  2.4e-07  4.1e-06   2.4e-07
    ddpm_late_start    x0_1    1.6e-06  1.9e-06  0.0e+00  1.3e-05  1.5e-06  2.8e-05   1.5e-06
    ddpm_no_white      final   2.0e-06  1.4e-06  0.0e+00  1.6e-05  2.0e-06  2.7e-05   2.0e-06
    ddpm_no_white      x0_1    6.5e-05  4.3e-05  0.0e+00  5.2e-04  4.3e-05  8.6e-04   4.3e-05
    ddpm_device_noise  final   1.2e-06  8.2e-07  6.1e-07  2.9e-05  3.7e-06  3.6e-05   3.7e-06
    ddpm_device_noise  x0_1    4.9e-05  4.0e-05  1.1e-05  7.5e-04  7.7e-05  1.1e-03   7.7e-05
    ddpm_group_a       final   2.4e-06  1.4e-06  0.0e+00  1.9e-05  1.9e-06  3.0e-05   1.9e-06
    ddpm_group_a       x0_1    6.4e-05  4.4e-05  0.0e+00  5.1e-04     -     8.7e-04      -
    ddpm_group_b       final   2.7e-06  1.6e-06  0.0e+00  2.1e-05  2.5e-06  3.5e-05   2.5e-06
    ddpm_group_b       x0_1    5.9e-05  5.3e-05  0.0e+00  4.7e-04     -     9.0e-04      -
    ddpm_batch_0       final   2.2e-06  1.3e-06  0.0e+00  1.8e-05  1.7e-06  2.8e-05   1.7e-06
    ddpm_batch_0       x0_1    7.0e-05  4.6e-05  0.0e+00  5.6e-04  5.1e-05  9.2e-04   5.1e-05
    ddpm_batch_1       final   2.6e-06  1.6e-06  0.0e+00  2.1e-05  2.3e-06  3.4e-05   2.3e-06
    ddpm_batch_1       x0_1    5.8e-05  4.5e-05  0.0e+00  4.7e-04  4.2e-05  8.3e-04   4.2e-05
    ddpm_dim128        final   2.2e-06  2.8e-06  0.0e+00  1.8e-05  2.1e-06  4.0e-05   2.7e-06
    ddpm_dim128        x0_1    5.4e-05  6.7e-05  0.0e+00  4.3e-04  5.0e-05  9.7e-04   6.8e-05
    edm_plain          final   1.4e-05  4.1e-07  0.0e+00  1.1e-04  9.0e-06  1.1e-04   9.0e-06
    edm_plain          x0_4    5.9e-01  2.3e-02  0.0e+00  4.8e+00  5.4e-01  4.9e+00   5.4e-01
    edm_no_clamp       final   1.6e-05  4.2e-07  0.0e+00  1.3e-04  1.5e-05  1.3e-04   1.5e-05
    edm_no_clamp       x0_4    9.1e-04  1.0e-05  0.0e+00  7.3e-03  9.1e-04  7.4e-03   9.1e-04
    edm_cfg            final   1.8e-05  4.3e-07  0.0e+00  1.4e-04  9.7e-06  1.5e-04   9.7e-06
    edm_cfg            x0_4    9.5e-01  2.3e-02  0.0e+00  7.6e+00  5.3e-01  7.8e+00   5.3e-01
    edm_late_start     final   1.6e-06  2.6e-07  0.0e+00  1.3e-05  1.5e-06  1.5e-05   1.5e-06
    edm_late_start     x0_3    2.7e-02  3.2e-03  0.0e+00  2.2e-01  1.5e-02  2.4e-01   1.5e-02
    edm_zero_init      final   8.1e-06  2.8e-07  0.0e+00  6.5e-05  6.3e-06  6.7e-05   6.3e-06
    edm_zero_init      x0_4    2.9e-01  2.0e-02  0.0e+00  2.3e+00  2.1e-01  2.5e+00   2.1e-01
    edm_sample_b2      final   1.4e-05  4.1e-07  0.0e+00  1.1e-04  1.2e-05  1.2e-04   1.2e-05
    edm_sample_b2      x0_4    5.3e-01  1.9e-02  0.0e+00  4.3e+00  3.7e-01  4.4e+00   3.7e-01
    edm_dpmpp_b1       final   1.6e-07  9.6e-08  0.0e+00  1.3e-06  1.5e-07  2.1e-06   1.5e-07
    edm_dpmpp_b1       img1    1.1e-05  1.5e-07  0.0e+00  8.4e-05  1.1e-05  8.5e-05   1.1e-05
    edm_dpmpp_b2       final   1.8e-07  1.3e-07  0.0e+00  1.4e-06  1.6e-07  2.5e-06   1.6e-07
    edm_dpmpp_b2       img1    9.6e-06  1.5e-07  0.0e+00  7.7e-05  9.6e-06  7.8e-05   9.6e-06
    bf16 one-step ddpm_plain     dim16    closest to its bound: img2 9.6e-07 / 5.6e-06; widest bound: x01 4.4e-06 / 1.4e-04
    bf16 one-step ddpm_cfg       dim16    closest to its bound: img4 3.9e-07 / 2.3e-06; widest bound: x01 1.8e-05 / 1.4e-04
    bf16 one-step ddpm_dim128    fusion1  closest to its bound: x02 6.9e-07 / 6.6e-06; widest bound: x01 1.8e-05 / 2.5e-04
    bf16 one-step ddpm_dim128    fusion0  closest to its bound: x02 8.6e-07 / 6.6e-06; widest bound: x01 2.7e-05 / 2.5e-04
    bf16 one-step edm_dpmpp_b2   dpmpp    closest to its bound: x01 1.1e-07 / 7.5e-07; widest bound: img1 7.0e-06 / 5.6e-05

bf16 Heun (EDM tiled_sample / sample) has no one-step check: its passes start from x_hat and the Euler point, which the wrappers do
not return.  Every distance is reported through test_engine_gpu._report.
"""
import os

import pytest
import torch

from oracle import srgd_oracle as O
from tests import sampler_cases as S
from tests.test_engine_gpu import G, _report

pytestmark = pytest.mark.gpu

_SAMPLERS = {}
LABEL = 1


def designed_sampler(dim, kind):
    """As test_engine_gpu.build_sampler / build_edm_sampler, with the designed state dict and a cache of its own."""
    key = ("designed", dim, kind)
    if key not in _SAMPLERS:
        import logging
        from srgd_amd.config import load_config
        from srgd_amd.model import get_model
        conf = load_config(os.path.join(os.path.dirname(G), "..", "conf", "conditional_continuous_linear_df8kost_dim128.yaml"))
        conf.unet_dim = dim
        conf.num_sample_steps = 50 if kind == "ddpm" else S.EDM.num_sample_steps
        if kind == "edm":
            conf.model = "conditional_elucidated"
        ema = get_model(conf, logging.getLogger("test"))
        sd = S.designed(dim, kind)[0]
        assert list(ema.module.state_dict().keys()) == list(sd.keys())
        ema.module.load_state_dict(sd, strict=True)
        _SAMPLERS[key] = ema.module.eval().to(torch.device("cuda"))
    return _SAMPLERS[key]


def _label():
    return torch.tensor([LABEL]).cuda()


def gpu_run(case, precision, **over):
    """The product's run of a case with trajectories, packed like ``sampler_cases.reference_run``'s tensors."""
    kind = "ddpm" if case["kind"] == "ddpm_tiled" else "edm"
    smp = designed_sampler(case["dim"], kind)
    cond = S.condition(case).cuda()
    kw = dict(case["kw"])
    kw.update(over)
    common = dict(condition_x=cond, class_label=_label(), num_sample_steps=case["steps"], precision=precision,
                  with_images=True, with_x0_images=True)
    smp.noise_source = "device" if case["device_noise"] else "host"
    smp.device_noise_seed = case["seed"]
    torch.manual_seed(case["seed"])
    try:
        if case["kind"].endswith("_tiled"):
            out, imgs, x0s = smp.tiled_sample(**common, **kw)
        elif case["kind"] == "edm_sample":
            out, imgs, x0s = smp.sample_org(batch_size=case["b"], **common, **kw)
        else:
            out, imgs, x0s = smp.sample_using_dpmpp(batch_size=case["b"], **common, **kw)
        torch.cuda.synchronize()
    finally:
        smp.noise_source = "host"
    assert len(imgs) == len(x0s) == len(S.executed_steps(case)) + 1
    return pack_gpu(out.cpu(), imgs, x0s)


def pack_gpu(out, imgs, x0s, image=None):
    sel = (lambda t: t) if image is None else (lambda t: t[image:image + 1])
    run = {"img0": sel(imgs[0])}
    for k in range(1, len(imgs)):
        run[f"img{k}"], run[f"x0_{k}"] = sel(imgs[k]), sel(x0s[k])
    run["final"] = sel(out)
    return run


def check_run(name, run, precision, **tags):
    ref, _ = S.reference(name)
    for k in ref:
        assert run[k].shape == ref[k].shape and run[k].dtype == torch.float32, (k, run[k].shape, ref[k].shape)
    return S.assert_run_within(run, ref, S.tolerances(name, precision),
                               report=lambda **kw: _report(test="sampler_exact", case=name, precision=precision, **kw), **tags)


# ------------------------------------------------------------------------------------------------ DDPM, whole runs
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["ddpm_plain", "ddpm_cfg", "ddpm_late_start", "ddpm_no_white", "ddpm_device_noise", "ddpm_dim128"])
def test_ddpm_tiled_run_matches_float64(name, precision):
    # (dim 16 has no layer the split-operand kernels take on the designed path - Cin % 32 != 0 - so f16x3 there is the fp32 route
    # under the other launch plan; ddpm_dim128 is where the operands are really split)
    check_run(name, gpu_run(S.CASE[name], precision), precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_class_guidance_is_an_exact_no_op_on_this_network(precision):
    # both passes of class guidance see the same eps on a network that ignores the label, and n + (e - n) g with e == n is n: the run
    # must equal the unguided one bit for bit.  Launches of 4 + 4 + 1 and 4 tiles: a pass stride off by a pixel or a tile breaks it.
    case = S.CASE["ddpm_plain"]
    smp = designed_sampler(16, "ddpm")
    outs = []
    for scale in (1.0, 2.0):
        torch.manual_seed(case["seed"])
        outs.append(smp.tiled_sample(batch_size=4, condition_x=S.condition(case).cuda(), class_label=_label(), num_sample_steps=3,
                                     class_cond_scale=scale, precision=precision, with_images=True, with_x0_images=True))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1] + outs[0][2], outs[1][1] + outs[1][2]):
        assert torch.equal(a, b)
    assert torch.isfinite(outs[0][0]).all()


# ------------------------------------------------------------------------------------------------ groups against the reference
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_mixed_size_seeded_group_matches_each_images_float64_run(precision):
    names = ["ddpm_group_a", "ddpm_group_b"]
    cases = [S.CASE[n] for n in names]
    smp = designed_sampler(16, "ddpm")
    outs = smp.tiled_sample(batch_size=4, condition_x=[S.condition(c).cuda() for c in cases], class_label=_label(),
                            num_sample_steps=cases[0]["steps"], seeds=[c["seed"] for c in cases], precision=precision)
    torch.cuda.synchronize()
    for name, out in zip(names, outs):
        ref, tol = S.reference(name)[0]["final"], S.tolerances(name, precision)["final"]
        d = S.distance(out.cpu(), ref)
        _report(test="sampler_exact", case=name, precision=precision, group="mixed_seeded", final=d, tolerance=tol)
        S.assert_close(out.cpu(), ref, tol, name)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_same_size_batch_matches_each_images_float64_run(precision):
    names = ["ddpm_batch_0", "ddpm_batch_1"]
    cases = [S.CASE[n] for n in names]
    smp = designed_sampler(16, "ddpm")
    torch.manual_seed(cases[0]["seed"])
    out, imgs, x0s = smp.tiled_sample(batch_size=4, condition_x=torch.cat([S.condition(c) for c in cases]).cuda(),
                                      class_label=_label(), num_sample_steps=cases[0]["steps"], precision=precision,
                                      with_images=True, with_x0_images=True)
    torch.cuda.synchronize()
    for i, name in enumerate(names):
        check_run(name, pack_gpu(out.cpu(), imgs, x0s, image=i), precision, group="batch", image=i)


# ------------------------------------------------------------------------------------------------ bf16: one step at a time
def _bf16_one_step_check(name, tag):
    case = S.CASE[name]
    _, M, b = S.designed(case["dim"], "ddpm")
    _, trace = S.reference(name)
    run = gpu_run(case, "bf16")
    (top, bottom, left, right), _, _ = S.geometry(case)
    crop = lambda t: t[:, :, top:bottom, left:right]
    cond = S.condition(case) * 2 - 1                      # fp32, one rounding: canvas_prepare_cond_kernel's value inside the image
    ts = torch.linspace(1.0, 0.0, case["steps"] + 1)
    worst = {}
    for k, i in enumerate(S.executed_steps(case)):
        prev = run["img0"] if k == 0 else crop(run[f"img{k}"])
        guided, scale = S._guided(case, i)
        step = lambda dt: S.ddpm_step(M, b, prev.to(dt), cond.to(dt), crop(trace["noise"][k]).to(dt), O.step_scalars(ts[i], ts[i + 1]),
                                      scale=scale, guided=guided, last=i == case["steps"] - 1, round_inputs=torch.bfloat16)
        want, want32 = step(torch.float64), step(torch.float32)
        for what, got, w64, w32 in (("img", crop(run[f"img{k + 1}"]), want[0], want32[0]),
                                    ("x0", crop(run[f"x0_{k + 1}"]), want[1], want32[1])):
            tol = S.one_step_tolerance(w32, w64)
            d = S.distance(got, w64)
            worst[f"{what}{k + 1}"] = (d, tol)
    _report(test="sampler_exact_one_step", case=name, precision="bf16", mode=tag, distance_and_tolerance=worst)
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad
    assert torch.isfinite(run["final"]).all()


@pytest.mark.parametrize("name", ["ddpm_plain", "ddpm_cfg"])
def test_bf16_every_step_matches_the_float64_step_on_rounded_inputs(name):
    _bf16_one_step_check(name, "dim16")


@pytest.mark.parametrize("fusion", ["1", "0"])
def test_bf16_dim128_steps_with_and_without_the_fused_output_convolution(fusion):
    # SRGD_FINAL_FUSION=1: conv1x1_bf16's EPI_GNTAIL_FINAL hands final_step 16 B per pixel (eps4); 0: the cooperative dot product
    smp = designed_sampler(128, "ddpm")
    try:
        os.environ["SRGD_FINAL_FUSION"] = fusion
        smp.model._invalidate_engines()
        _bf16_one_step_check("ddpm_dim128", "fusion" + fusion)
    finally:
        os.environ.pop("SRGD_FINAL_FUSION", None)
        smp.model._invalidate_engines()


def test_bf16_dpmpp_every_step_matches_the_float64_step_on_rounded_inputs():
    # the one EDM loop whose step starts from what the wrapper returns: the canvas itself (c_in x is ONE fp32 product, reproduced
    # bit for bit before the bfloat16 rounding) and the previous denoised image, which is the model's on the previous canvas.  The
    # Heun loops' passes start from x_hat and the Euler point, which stay inside the engine: no one-step check, bf16 left out.
    name = "edm_dpmpp_b2"
    case = S.CASE[name]
    _, M, b = S.designed(16, "edm")
    run = gpu_run(case, "bf16")
    cond = S.condition(case) * 2 - 1
    n, steps = case["steps"], S.executed_steps(case)
    worst = {}
    for k, i in enumerate(steps):
        sc = S.dpmpp_scalars(S.EDM, n, i, steps[0])

        def step(dt):
            old = None
            if sc["gamma"] is not None:
                p = S.dpmpp_scalars(S.EDM, n, i - 1, steps[0])
                old = S._edm_denoise(M, b, run[f"img{k - 1}"].to(dt), cond.to(dt), p["c_in"], p["c_skip"], p["c_out"], 1.0, False,
                                     True, torch.bfloat16)
            return S.edm_dpmpp_step(M, b, run[f"img{k}"].to(dt), cond.to(dt), old, sc, round_inputs=torch.bfloat16)
        want, want32 = step(torch.float64), step(torch.float32)
        for what, got, w64, w32 in (("img", run[f"img{k + 1}"], want[0], want32[0]), ("x0", run[f"x0_{k + 1}"], want[1], want32[1])):
            worst[f"{what}{k + 1}"] = (S.distance(got, w64), S.one_step_tolerance(w32, w64))
    _report(test="sampler_exact_one_step", case=name, precision="bf16", mode="dpmpp", distance_and_tolerance=worst)
    assert sum(S.dpmpp_scalars(S.EDM, n, i, steps[0])["gamma"] is not None for i in steps) >= 2      # the history term is exercised
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad
    assert torch.isfinite(run["final"]).all()


# ------------------------------------------------------------------------------------------------ EDM, whole runs
@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["edm_plain", "edm_no_clamp", "edm_cfg", "edm_late_start", "edm_zero_init", "edm_sample_b2",
                                  "edm_dpmpp_b1", "edm_dpmpp_b2"])
def test_edm_run_matches_float64(name, precision):
    check_run(name, gpu_run(S.CASE[name], precision), precision)
