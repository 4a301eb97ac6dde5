"""CPU checks of tests/sampler_cases.py: the designed network is what it claims to be, the oracle's ``unet=`` hook is neutral, every
tolerance the GPU file uses comes from the oracle alone, and the assertions reject wrong samplers.

``python -m pytest tests/test_sampler_cases_cpu.py -s`` prints, per case and compared tensor, E32, E_split, E_noise and the
resulting fp32 / f16x3 tolerances.
"""
import pytest
import torch

from oracle import philox as P
from oracle import srgd_oracle as O
from srgd_amd.synth import synth_state_dict
from tests import sampler_cases as S

NAMES = [c["name"] for c in S.CASES]
EDM_HEUN = [c["name"] for c in S.CASES if c["kind"] in ("edm_tiled", "edm_sample")]


# ------------------------------------------------------------------------------------------------ the construction
@pytest.mark.parametrize("kind", ["ddpm", "edm"])
@pytest.mark.parametrize("dim", [16, 128])
def test_designed_weights_are_exact_in_bf16_and_f16_and_mix_channels(dim, kind):
    sd, M, b = S.designed(dim, kind)
    pre = "model." if kind == "ddpm" else "net."
    for key in ("init_conv.weight", "final_res_block.res_conv.weight", "final_conv.weight", "final_conv.bias"):
        w = sd[pre + key]
        assert torch.equal(w.to(torch.bfloat16).float(), w) and torch.equal(w.to(torch.float16).float(), w), key
    for key in ("init_conv.bias", "final_res_block.res_conv.bias", "final_res_block.block2.norm.weight",
                "final_res_block.block2.norm.bias"):
        assert not sd[pre + key].any(), key
    a = sd[pre + "init_conv.weight"]
    assert (a != 0).sum() == dim and (a[:, :, 3, 3] != 0).sum() == dim                 # one plane per hidden channel, centre tap
    assert ((a[a != 0]).log2() % 1 == 0).all()                                          # power-of-two gains
    r = sd[pre + "final_res_block.res_conv.weight"]
    assert not r[:, :dim].any() and (r != 0).sum() == dim and ((r[r != 0]).log2() % 1 == 0).all()
    assert (M != 0).sum() >= 16, M                                                      # M mixes the channels
    assert (M[:, 3:].abs().sum(0) > 0).all() and M[:, 3:].abs().max() >= 2.0 ** -6      # the condition is visible to guidance
    # everything else is the random network: nothing but the named tensors was touched
    base = synth_state_dict(S.schema(dim, pre), seed=0)
    touched = {k for k in sd if not torch.equal(sd[k], base[k])}
    assert touched <= {pre + k for k in ("init_conv.weight", "init_conv.bias", "final_res_block.res_conv.weight",
                                         "final_res_block.res_conv.bias", "final_res_block.block2.norm.weight",
                                         "final_res_block.block2.norm.bias", "final_conv.weight", "final_conv.bias")}


@pytest.mark.parametrize("dim", [16, 128])
def test_the_designed_network_is_the_closed_form(dim):
    """``unet_forward`` with the designed weights against M [x; cond] + b, with and without condition and label.

    Tolerance.  The centre tap and ``res_conv`` multiply one value by a power of two: exact.  The zeroed GroupNorm gives
    silu(0) = 0 exactly, so the last block's output is r times a power of two.  What rounds is ``final_conv``: a sum of ``dim``
    exact-in-fp32 products and the bias.  Summed in blocks or pairs its error is at most about log2(dim) + 1 <= 8 roundings of
    2^-24 relative to sum |terms| = (|F| |R| |A|) |[x; cond]| + |b|, i.e. 4 ulp (of 2^-23) of that per-pixel magnitude."""
    sd, M, b = S.designed(dim, "ddpm")
    usd = O.strip_model_prefix(sd)
    a = usd["init_conv.weight"][:, :, 3, 3].double().abs()
    r = usd["final_res_block.res_conv.weight"][:, dim:, 0, 0].double().abs()
    f = usd["final_conv.weight"][:, :, 0, 0].double().abs()
    m_abs = f @ r @ a
    g = torch.Generator().manual_seed(dim)
    x = torch.randn(2, 3, 16, 16, generator=g) * 3
    cond = torch.rand(2, 3, 16, 16, generator=g) * 2 - 1
    ls = torch.tensor([0.3, -2.0])
    for c in (cond, None):
        mag = torch.einsum("oi,bihw->bohw", m_abs[:, :3], x.double().abs()) + b.abs().view(1, 3, 1, 1)
        if c is not None:
            mag = mag + torch.einsum("oi,bihw->bohw", m_abs[:, 3:], c.double().abs())
        want = S.pointwise_eps(M, b, x, c, torch.float64)
        for label in (torch.tensor([1]), None):
            with torch.inference_mode():
                got = O.unet_forward(usd, O.UnetCfg(dim=dim), x, ls, label, c)
            err = (got.double() - want).abs()
            assert torch.isfinite(got).all()
            assert (err <= 4 * 2.0 ** -23 * mag).all(), (dim, c is None, label, float((err / mag).max()) * 2 ** 23)
    assert float(want.abs().max()) > 1.0                                                # a visible eps, not a vanishing one


def test_the_unet_hook_and_the_trace_are_neutral():
    # one tile, random weights, the real network: default call == hooked + traced call, bit for bit
    sd = O.strip_model_prefix(synth_state_dict(S.schema(16), seed=0))
    cond = S._rand_cond(256, 256, 99)
    kw = dict(num_sample_steps=2, cond_scale=1.5)
    with torch.inference_mode():
        torch.manual_seed(7)
        plain = O.tiled_sample(sd, O.UnetCfg(dim=16), cond, torch.tensor([1]), **kw)
        torch.manual_seed(7)
        trace = {}
        hooked = O.tiled_sample(sd, O.UnetCfg(dim=16), cond, torch.tensor([1]), trace=trace,
                                unet=lambda *a: O.unet_forward(*a), **kw)
    assert torch.equal(plain, hooked) and plain.dtype == torch.float32
    assert len(trace["img"]) == len(trace["noise"]) == len(trace["ring"]) == 2
    assert trace["noise"][0].abs().max() > 1 and not trace["noise"][1].any() and trace["ring"][1] is not None


def test_a_replay_reproduces_the_recording_run():
    # NoiseSource(record=True) keeps copies and ReplayNoise hands copies out: tiled_sample writes tiles into its start draw in place
    case = S.CASE["ddpm_no_white"]
    _, M, b = S.designed(16, "ddpm")
    run = lambda noise, trace: O.tiled_sample({}, O.UnetCfg(dim=16), S.condition(case), None, num_sample_steps=3, noise=noise,
                                              trace=trace, unet=S.closed_unet(M, b))
    with torch.inference_mode():
        torch.manual_seed(3)
        rec, t0, t1, t2 = O.NoiseSource(record=True), {}, {}, {}
        first = run(rec, t0)
        torch.manual_seed(3)
        assert torch.equal(rec.draws[0], torch.randn(1, 3, 256, 256))                   # the recording survived the run
        replay = O.ReplayNoise(rec.draws)
        second = run(replay, t1)
        third = run(O.ReplayNoise(replay.draws), t2)                                    # and the replay survived its run
    assert replay.i == len(rec.draws)
    for other, t in ((second, t1), (third, t2)):
        assert torch.equal(first, other)
        assert all(torch.equal(a, b_) for a, b_ in zip(t0["img"] + t0["x_start"], t["img"] + t["x_start"]))


def test_one_tile_device_plan_is_the_oracles_draw_plan():
    case = S.CASE["ddpm_device_noise"]
    mine = S.one_tile_device_plan(case["seed"], case["steps"])
    plan = P.device_noise_draws("ddpm_tiled", seed=case["seed"], num_sample_steps=case["steps"], height=256, width=256,
                                batch_size=case["kw"]["batch_size"])
    assert len(mine) == len(plan) and all(torch.equal(a, b) for a, b in zip(mine, plan))


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("name", NAMES)
def test_runs_are_dtype_clean_and_the_canvas_recurrence_is_the_oracles_run(name):
    case = S.CASE[name]
    ref, trace = S.reference(name)
    assert all(v.dtype == torch.float64 for v in ref.values())
    assert len(ref) == 2 * len(S.executed_steps(case)) + 2
    again = S.canvas_run(case, trace)
    d = S.distances(again, ref)
    assert max(d.values()) <= 1e-12, d                    # the same float64 operations (0 in practice)


@pytest.mark.parametrize("name", NAMES)
def test_tolerances_come_from_the_oracle_alone(name, capsys):
    case = S.CASE[name]
    ref, _ = S.reference(name)
    m = S.measured(name)
    tol32, tol3 = S.tolerances(name, "fp32"), S.tolerances(name, "f16x3")
    with capsys.disabled():
        print(f"\n{name}")
        for k in ref:
            print(f"  {k:6s} max|ref| {float(ref[k].abs().max()):9.3e}  E32 {m[k]['e32']:.2e}  E_split {m[k]['e_split']:.2e}  "
                  f"E_noise {m[k]['e_noise']:.2e}  floor {m[k]['floor']:.2e}  tol fp32 {tol32[k]:.2e}  tol f16x3 {tol3[k]:.2e}")
    for k in ref:
        assert 0 <= m[k]["e32"] < float("inf") and 0 <= m[k]["e_split"] < float("inf")
        assert tol32[k] == max(S.MARGIN * m[k]["e32"] + S.DEVICE_NOISE_MARGIN * m[k]["e_noise"], m[k]["floor"])
        assert tol3[k] == max(S.MARGIN * (m[k]["e32"] + m[k]["e_split"]) + S.DEVICE_NOISE_MARGIN * m[k]["e_noise"], m[k]["floor"])
        assert m[k]["floor"] == 4 * S.ulp32(float(ref[k].abs().max()))
        # a tolerance is a rounding-level quantity, far below the tensor's magnitude (the widest: x_start of the first step, where
        # 1 / alpha = 150 multiplies the roundings of a canvas of magnitude 5, and EDM's last slopes, divided by sigma_next = 0.002)
        assert tol3[k] <= 1e-2 * max(float(ref[k].abs().max()), 1e-30) or not ref[k].any(), (k, tol3[k])
    assert m["final"]["e32"] > 0 and (m["final"]["e_noise"] > 0) == case["device_noise"]
    # inside the 1e-3 bar the whole-run tests hold final images to: ten times for DDPM; EDM's canvases reach magnitude 400 on the way
    assert tol3["final"] <= (1e-4 if case["kind"] == "ddpm_tiled" else 5e-4)


# ------------------------------------------------------------------------------------------------ the assertions have teeth
@pytest.mark.parametrize("mutant", list(S.MUTANTS))
def test_a_wrong_sampler_misses_its_case_by_a_factor_of_100(mutant):
    name = S.MUTANTS[mutant]
    case = S.CASE[name]
    ref, trace = S.reference(name)
    wrong = S.canvas_run(case, trace, mutant=mutant)
    factor = S.miss_factor(wrong, ref, S.tolerances(name, "f16x3"))      # the wider of the two whole-run tolerances
    assert factor >= S.MUTANT_FACTOR, (mutant, factor)
    with pytest.raises(AssertionError):
        S.assert_run_within(wrong, ref, S.tolerances(name, "f16x3"))


def test_the_bf16_model_is_far_from_the_exact_one_and_the_one_step_bound_is_sharp():
    # what the one-step check of the bf16 mode can see: rounding [x; cond] moves a step by ~1e-2, its tolerance is ~1e-5
    case = S.CASE["ddpm_plain"]
    _, M, b = S.designed(16, "ddpm")
    ref, trace = S.reference("ddpm_plain")
    (top, bottom, left, right), _, _ = S.geometry(case)
    crop = lambda t: t[:, :, top:bottom, left:right]
    ts = torch.linspace(1.0, 0.0, case["steps"] + 1)
    prev, cond = crop(ref["img2"]).float(), S.condition(case) * 2 - 1
    step = lambda dt, rnd: S.ddpm_step(M, b, prev.to(dt), cond.to(dt), crop(trace["noise"][2]).to(dt),
                                       O.step_scalars(ts[2], ts[3]), round_inputs=rnd)
    exact, model, model32 = step(torch.float64, None), step(torch.float64, torch.bfloat16), step(torch.float32, torch.bfloat16)
    tol = S.one_step_tolerance(model32[0], model[0])
    assert S.distance(exact[0], model[0]) >= 100 * tol
    assert tol <= 1e-4


# ------------------------------------------------------------------------------------------------ saturation
@pytest.mark.parametrize("name", NAMES)
def test_at_most_a_quarter_of_the_last_compared_pixels_sit_on_the_clamp(name):
    """DDPM: the final image and x_start after the last step.  EDM DPM-Solver++: the final image.  EDM Heun: a few-step Heun run
    from sigma = 80 overshoots for every pointwise-linear network tried (diagonal of M from -2.5 to 1.25: 60 - 95 % of the final
    image on the clamp), so there the unclamped canvas after the last step is compared as well - nothing of it sits on a clamp -
    and the cap is asserted on the denoiser's clamp instead: the share of that canvas outside [-1, 1] is what the final image's
    clamp hides, and every such pixel is compared unclamped."""
    case = S.CASE[name]
    ref, _ = S.reference(name)
    last = len(S.executed_steps(case))
    if name in EDM_HEUN:
        assert torch.isfinite(ref[f"img{last}"]).all() and f"img{last}" in S.tolerances(name, "fp32")
        return
    assert S.saturated_share(ref["final"], 0.0, 1.0) <= S.SATURATION_CAP
    if case["kind"] == "ddpm_tiled":
        (top, bottom, left, right), _, _ = S.geometry(case)
        assert S.saturated_share(ref[f"x0_{last}"][:, :, top:bottom, left:right], -1.0, 1.0) <= S.SATURATION_CAP
        first = ref["x0_1"][:, :, top:bottom, left:right]
        if case["kw"].get("generation_start_steps", 0) == 0 and case["kw"].get("start_white_noise", True):
            assert S.saturated_share(first, -1.0, 1.0) >= 0.5         # and the clamped branch is exercised at the start
