"""Precision schedules on the MI355X (``tiled_sample(precision_schedule=...)``, srgd_amd.precision_schedule) on the dim-16 model of
tests/guidance_cases.py: a single-name schedule is the plain run, the head of a mixed run is the head's run, a step depends only on
the canvas before it and on its own precision, a mixed run of the two parity modes against the reference's fixture on host noise,
lanes, lock-step groups and the combination with the few-step sampler and the dynamic threshold.  The condition is 300 x 260 (four
even tiles, one odd tile and a ring), runs take 6 steps on device noise, comparisons are on the int32 bit patterns."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import guidance_cases as G
from tests.golden import cases as C

pytestmark = pytest.mark.gpu
LABEL = torch.tensor([G.LABEL])
SEED = 41
MIXED = "bf16:3,f16x3"


def _sampler(noise="device"):
    from tests.test_engine_gpu import build_sampler
    sampler = build_sampler(G.DIM)
    sampler.noise_source = noise
    return sampler


def _run(model, seed, **kw):
    """One call after seeding both noise sources; the model is the session's shared one and leaves with host noise again."""
    torch.manual_seed(seed)
    model.device_noise_seed = seed
    try:
        return model.tiled_sample(class_label=LABEL.cuda(), **kw)
    finally:
        model.noise_source = "host"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _cond(h=300, w=260, seed=19):
    return torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(seed)).cuda()


@functools.lru_cache(maxsize=None)
def _trajectory(kind, name, steps=6, **extra):
    """(output, canvases, predictions, precision log) of one run on the shared condition, as CPU tensors - made once per session and
    read-only; ``kind``: "precision" or "precision_schedule"."""
    log = []
    out, xts, x0s = _run(_sampler(), SEED, batch_size=8, condition_x=_cond(), num_sample_steps=steps, with_images=True,
                         with_x0_images=True, precision_log=log, **{kind: name}, **extra)
    torch.cuda.synchronize()
    assert len(xts) == len(x0s) == steps + 1
    return out.cpu(), xts, x0s, tuple(log)


def _same(a, b, entries):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in entries)


# ------------------------------------------------------------------------------------------- 1. a single name
@pytest.mark.parametrize("name", ["bf16", "f16x3"])
def test_a_single_name_schedule_is_the_plain_run(name):
    plain = _trajectory("precision", name)
    for spec in (name, f"{name}:6", ((name, 2), (name, None))):
        got = _trajectory("precision_schedule", spec)
        assert torch.equal(_bits(got[0]), _bits(plain[0])), spec
        assert _same(got[1], plain[1], range(7)) and _same(got[2], plain[2], range(7)), spec
        assert got[3] == plain[3] == (name,) * 6


# ------------------------------------------------------------------------------------------- 2. the head
def test_the_head_of_a_mixed_run_is_the_heads_run():
    head = _trajectory("precision", "bf16")
    mixed = _trajectory("precision_schedule", MIXED)
    assert mixed[3] == ("bf16",) * 3 + ("f16x3",) * 3
    for k in (1, 2):                                                     # canvases and predictions
        assert _same(mixed[k], head[k], range(4))
        assert not torch.equal(_bits(mixed[k][4]), _bits(head[k][4]))    # the first f16x3 step
    assert torch.isfinite(mixed[0]).all()
    # the wrapper's attribute is the keyword's default, and ``precision=`` of a call overrides the attribute
    model = _sampler()
    model.precision_schedule = MIXED
    try:
        log = []
        out = _run(model, SEED, batch_size=8, condition_x=_cond(), num_sample_steps=6, precision_log=log)
        assert log == list(mixed[3]) and torch.equal(_bits(out), _bits(mixed[0]))
        model.noise_source = "device"
        out = _run(model, SEED, batch_size=8, condition_x=_cond(), num_sample_steps=6, precision="bf16")
        assert torch.equal(_bits(out), _bits(head[0]))
    finally:
        model.precision_schedule = None


# ------------------------------------------------------------------------------------------- 3. a step and its canvas
def test_a_step_depends_only_on_the_canvas_before_it_and_on_its_own_precision():
    mixed = _trajectory("precision_schedule", MIXED)
    back = _trajectory("precision_schedule", "bf16:3,f16x3:1,bf16")
    assert back[3] == ("bf16",) * 3 + ("f16x3",) + ("bf16",) * 2
    for k in (1, 2):
        assert _same(back[k], mixed[k], range(5))
        assert not torch.equal(_bits(back[k][5]), _bits(mixed[k][5]))
    tail = _trajectory("precision", "f16x3")
    front = _trajectory("precision_schedule", "f16x3:1,bf16")
    assert front[3] == ("f16x3",) + ("bf16",) * 5
    for k in (1, 2):
        assert _same(front[k], tail[k], range(2))
        assert not torch.equal(_bits(front[k][2]), _bits(tail[k][2]))


# ------------------------------------------------------------------------------------------- 4. the reference
def test_the_two_parity_modes_mixed_stay_within_the_bar_of_the_reference():
    """Host noise, condition guidance from step 2 on, fp32 for the first S // 2 steps and f16x3 for the rest: the host-noise draw
    order and the guidance survive the switch.  Bar: 1e-3 on the final pixels, the project's, which either mode alone meets on this
    fixture (tests/test_engine_gpu.py::test_tiled_sample_fp32_matches_reference)."""
    from tests.test_engine_gpu import _report, build_sampler
    case = next(c for c in C.SAMPLER_CASES if c["name"] == "dim16_300x300_lrcfg")
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"sample_{case['name']}.npz"))
    sampler = build_sampler(case["dim"], weight_seed=case["weight_seed"])
    steps = case["steps"]
    spec = f"fp32:{steps // 2},f16x3"
    torch.manual_seed(case["seed"])
    assert np.array_equal(torch.randn(16).numpy(), z["first_draw"]), "torch CPU generator stream differs from the fixture's"
    torch.manual_seed(case["seed"])
    sampler.noise_source = "host"
    log = []
    got = sampler.tiled_sample(batch_size=case["batch_size"], condition_x=C.sampler_condition(case).cuda(),
                               class_label=torch.tensor([case["label"]]).cuda(), cond_scale=case["cond_scale"],
                               class_cond_scale=case["class_cond_scale"], num_sample_steps=steps, precision_schedule=spec,
                               precision_log=log, **C.extra_kwargs(case))
    torch.cuda.synchronize()
    want = torch.from_numpy(z["image"])
    assert got.shape == want.shape and got.dtype == torch.float32
    assert log == ["fp32"] * (steps // 2) + ["f16x3"] * (steps - steps // 2)
    err = (got.cpu() - want).abs().max().item()
    _report(test="tiled_sample", case=case["name"], precision_schedule=spec, max_abs=err)
    print(f"precision schedule {spec} on {case['name']}: max-abs {err:.3e}")
    assert err <= 1e-3, err


# ------------------------------------------------------------------------------------------- 5. lanes
def test_two_step_lanes_change_no_bit_of_a_mixed_run():
    model = _sampler()
    cond = C.synthetic_lr_condition(0, 256, 256).cuda()                 # 25 / 16 tiles per step, as the lanes test of the engine suite
    keep = model.step_lanes
    outs = []
    try:
        for lanes in (1, 2):
            model.step_lanes = lanes
            model.noise_source = "device"
            outs.append(_run(model, 5, batch_size=25, condition_x=cond, num_sample_steps=6, precision_schedule=MIXED).cpu())
    finally:
        model.step_lanes = keep
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.isfinite(outs[0]).all()


# ------------------------------------------------------------------------------------------- 6. lock-step
def test_a_lock_step_group_is_its_solo_runs():
    conds = [_cond(), _cond(256, 256, 23)]
    kw = dict(batch_size=6, num_sample_steps=6, precision_schedule=MIXED)
    solo = [_run(_sampler(), SEED, condition_x=c, **kw) for c in conds]
    log = []
    group = _run(_sampler(), SEED, condition_x=conds, precision_log=log, **kw)
    assert log == ["bf16"] * 3 + ["f16x3"] * 3
    for k in range(2):
        assert torch.equal(_bits(group[k]), _bits(solo[k])), k
    seeded = _run(_sampler(), 1, condition_x=conds, seeds=[SEED, SEED + 1], **kw)
    assert torch.equal(_bits(seeded[0]), _bits(solo[0]))
    assert torch.equal(_bits(seeded[1]), _bits(_run(_sampler(), SEED + 1, condition_x=conds[1], **kw)))


# ------------------------------------------------------------------------------------------- 7. combinations
def test_the_few_step_sampler_and_the_threshold_combine_with_a_schedule():
    extra = dict(sampler="dpmpp2m", dynamic_threshold=0.995)
    head = _trajectory("precision", "bf16", 4, **extra)
    mixed = _trajectory("precision_schedule", MIXED, 4, **extra)
    assert mixed[3] == ("bf16",) * 3 + ("f16x3",)
    for k in (1, 2):
        assert _same(mixed[k], head[k], range(4))
    assert torch.isfinite(mixed[0]).all() and float(mixed[0].min()) >= 0.0 and float(mixed[0].max()) <= 1.0


# ------------------------------------------------------------------------------------------- 8. reported, not gated
def test_the_distance_of_a_mixed_run_to_fp32_is_reported():
    """Random dim-16 weights say nothing about the curve (tools/price_precision_schedule.py measures it on the reference's
    fixtures): the figures are printed, the output is only finite and in [0, 1]."""
    from tests.test_engine_gpu import _report
    exact = _trajectory("precision", "fp32")[0]
    mixed, head = _trajectory("precision_schedule", MIXED)[0], _trajectory("precision", "bf16")[0]
    err_mixed, err_head = float((mixed - exact).abs().max()), float((head - exact).abs().max())
    _report(test="precision_schedule_vs_fp32", schedule=MIXED, max_abs=err_mixed, bf16_max_abs=err_head)
    print(f"max-abs against fp32 after 6 steps: {MIXED} {err_mixed:.3e}, bf16 {err_head:.3e}")
    assert torch.isfinite(mixed).all() and float(mixed.min()) >= 0.0 and float(mixed.max()) <= 1.0
