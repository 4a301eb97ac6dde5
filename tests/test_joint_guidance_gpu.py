"""Joint guidance on the GPU: ``tiled_sample(joint_guidance=True)`` -> srgd_sampler_step with passes = 3 -> final_step_kernel<T, true>, against
the yardsticks of tests/joint_guidance_cases.py.

1. closed-form network (the label cannot reach eps: the third term of the combine is exactly zero): one joint step on the even and
   one on the odd grid against the float64 condition-guided run, ``sampler_cases``' own tolerances; bf16 one step at a time;
2. random weights, one joint step from a random canvas on host noise: img and x_start against the float64 step of the product's own
   three U-Net evaluations; the bar is 4 x the larger deviation of the parent's two two-pass steps under the same construction,
   measured in the test;
3. end to end against the restated oracle loop on host noise (an unguided, a class-guided and two joint steps);
4. bit-identities (mixed group, grouping, graphs, lanes, seeds);  5. one active scale: the run without the keyword, byte for byte;
6. the C ABI's refusals;  7. composition with the dynamic threshold and DDIM in bf16.

Every figure goes through test_engine_gpu._report before anything is asserted."""
import ctypes as CT
import os

import pytest
import torch

from oracle import srgd_oracle as O
from tests import joint_guidance_cases as J
from tests import sampler_cases as S
from tests.test_engine_gpu import _report, build_edm_sampler, build_sampler
from tests.test_sampler_exact_gpu import designed_sampler, pack_gpu

pytestmark = pytest.mark.gpu
JOINT = dict(cond_scale=J.S_C, class_cond_scale=J.S_L, joint_guidance=True)


def _label(v=J.LABEL):
    return torch.tensor([v]).cuda()


def _sampler():
    return build_sampler(J.DIM, weight_seed=J.WEIGHT_SEED)


# ------------------------------------------------------------------------------------------------ 1. closed form
def _closed_form_run(key, precision):
    case = J.closed_form_case(key)
    smp = designed_sampler(case["dim"], "ddpm")
    torch.manual_seed(case["seed"])
    out, imgs, x0s = smp.tiled_sample(batch_size=4, condition_x=S.condition(case).cuda(), class_label=_label(),
                                      num_sample_steps=case["steps"], precision=precision, with_images=True, with_x0_images=True,
                                      cond_scale=J.SENS_S_C, class_cond_scale=J.SENS_S_L, joint_guidance=True)
    torch.cuda.synchronize()
    return pack_gpu(out.cpu(), imgs, x0s)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("key", ["img256", "img300"])
def test_closed_form_joint_steps_match_the_float64_condition_guided_run(key, precision):
    ref, _ = J.closed_form_reference(key)
    S.assert_run_within(_closed_form_run(key, precision), ref, J.closed_form_tolerances(key, precision),
                        report=lambda **kw: _report(test="joint_closed_form", case=key, precision=precision, **kw))


@pytest.mark.parametrize("key", ["img256", "img300"])
def test_closed_form_joint_steps_bf16_one_step_at_a_time(key):
    # as test_sampler_exact_gpu._bf16_one_step_check: the float64 step on bfloat16-rounded [x; cond] of the GPU's own previous canvas
    case = J.closed_form_case(key)
    _, M, b = S.designed(case["dim"], "ddpm")
    _, trace = J.closed_form_reference(key)
    run = _closed_form_run(key, "bf16")
    (top, bottom, left, right), _, _ = S.geometry(case)
    crop = lambda t: t[:, :, top:bottom, left:right]
    cond = S.condition(case) * 2 - 1
    ts = torch.linspace(1.0, 0.0, case["steps"] + 1)
    worst = {}
    for k in range(case["steps"]):
        prev = run["img0"] if k == 0 else crop(run[f"img{k}"])
        step = lambda dt: S.ddpm_step(M, b, prev.to(dt), cond.to(dt), crop(trace["noise"][k]).to(dt), O.step_scalars(ts[k], ts[k + 1]),
                                      scale=J.SENS_S_C, guided=True, last=k == case["steps"] - 1, round_inputs=torch.bfloat16)
        want, want32 = step(torch.float64), step(torch.float32)
        for what, got, w64, w32 in (("img", crop(run[f"img{k + 1}"]), want[0], want32[0]), ("x0", crop(run[f"x0_{k + 1}"]), want[1], want32[1])):
            worst[f"{what}{k + 1}"] = (S.distance(got, w64), S.one_step_tolerance(w32, w64))
    _report(test="joint_closed_form_one_step", case=key, precision="bf16", distance_and_tolerance=worst)
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad
    assert torch.isfinite(run["final"]).all()


# ------------------------------------------------------------------------------------------------ 2. one step, random weights
def _begin(eng, cond01, class_id, steps):
    """``srgd_sampler_begin`` of a [1,3,h,w] condition as ``tiled_sample`` makes it -> (condition canvas, even tile boxes, step table,
    log-SNRs)."""
    from srgd_amd._lib import SamplerGeometry
    from srgd_amd.model import _schedule_of, get_area, get_coord_and_pad, get_coords
    _, _, h, w = cond01.shape
    (left, top, _, _), pad = get_coord_and_pad(h, w)
    hp, wp = h + pad[2] + pad[3], w + pad[0] + pad[1]
    c0 = get_coords(hp, wp, 256, 256, diff=0)
    c1 = c0 if hp <= 256 and wp <= 256 else get_coords(hp - 256, wp - 256, 256, 256, diff=128)
    (sl, st, sr, sb), _ = get_area(c1, hp, wp)
    geo = SamplerGeometry(H=h, W=w, Hp=hp, Wp=wp, left=left, top=top, inner_l=sl, inner_t=st, inner_r=sr, inner_b=sb, tile=256,
                          n_even=len(c0), n_odd=len(c1), n_images=1)
    scalars, log_snrs = _schedule_of(steps, None)
    canvas = torch.empty(1, 3, hp, wp, device="cuda")
    eng.sampler_begin(geo, cond01, canvas, [(a, c) for (a, _, c, _) in c0], [(a, c) for (a, _, c, _) in c1], scalars, log_snrs, class_id)
    return canvas, c0, scalars, log_snrs


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_one_joint_step_matches_the_float64_step_of_the_products_three_evaluations(precision):
    smp = _sampler()
    eng = smp.model.engine(precision)
    i, n = J.ONE_STEP_INDEX, J.ONE_STEP_STEPS
    img0, c01, z = (t.cuda() for t in J.one_step_inputs(300, 300))
    canvas, boxes, scalars, log_snrs = _begin(eng, c01, J.LABEL, n)
    assert len(boxes) == 9 and i % 2 == 0
    gather = lambda t: torch.cat([t[:, :, a:b, c:d] for (a, b, c, d) in boxes], 0)
    x, cnd = gather(img0), gather(canvas)
    ls = torch.full((len(boxes),), float(log_snrs[i]))
    keep = smp.model.precision
    try:                                                   # the existing U-Net forward, in the precision under test
        smp.model.precision = precision
        e, n_c, n_l = smp.model(x, ls, _label(), cnd), smp.model(x, ls, _label(), None), smp.model(x, ls, None, cnd)
    finally:
        smp.model.precision = keep
    sc = {k: float(getattr(scalars[i], k)) for k in ("alpha", "sigma", "alpha_next", "c", "one_minus_c", "noise_scale")}
    s_c, s_l = J.SENS_S_C, J.SENS_S_L
    eps = {"joint": J.combine64(e, n_c, n_l, s_c, s_l), "class": J.class_guided64(e, n_l, s_l), "cond": J.cond_guided64(e, n_c, s_c)}
    dev = {}
    for mode in ("class", "cond", "joint"):
        canvas, _, _, _ = _begin(eng, c01, J.LABEL, n)
        img, xs = img0.clone(), torch.zeros_like(img0)
        if mode == "joint":
            eng.sampler_step_joint(i, img, canvas, xs, z, None, s_c, s_l, 4)       # launches of 4, 4, 1 tiles
        else:
            eng.sampler_step(i, img, canvas, xs, z, None, 2, 1 if mode == "class" else 2, s_l if mode == "class" else s_c, 4)
        torch.cuda.synchronize()
        want_img, want_x0 = J.step64(x, eps[mode], z, sc)
        dev[mode] = dict(img=S.distance(gather(img), want_img), x_start=S.distance(gather(xs), want_x0))
        assert float((want_x0.abs() < 1).double().mean()) > 0.25
    # a three-term combine carries at most two scaled differences where the parent's carries one; x 2 is headroom
    bar = {k: 4 * max(dev["class"][k], dev["cond"][k]) for k in ("img", "x_start")}
    _report(test="joint_one_step", precision=precision, deviations=dev, bar=bar)
    print("one joint step", precision, dev, "bar", bar)
    assert 0 < bar["x_start"] <= J.ONE_STEP_BAR_CAP, bar     # the cap tests/test_joint_guidance_cpu.py's sensitivity test rests on
    for k in ("img", "x_start"):
        assert dev["joint"][k] <= bar[k], (k, dev, bar)


# ------------------------------------------------------------------------------------------------ 3. end to end
def _e2e(smp, precision, **over):
    e = J.E2E
    kw = dict(batch_size=e["batch_size"], condition_x=J.condition(*e["size"]).cuda(), class_label=_label(), num_sample_steps=e["steps"],
              cond_scale=e["cond_scale"], class_cond_scale=e["class_cond_scale"], guidance_start_steps=e["guidance_start_steps"],
              class_guidance_start_steps=e["class_guidance_start_steps"], joint_guidance=True, precision=precision)
    kw.update(over)
    torch.manual_seed(e["seed"])
    out = smp.tiled_sample(**kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_end_to_end_against_the_restated_oracle_loop(precision):
    want, trace = J.e2e_oracle()
    out, imgs, x0s = _e2e(_sampler(), precision, with_images=True, with_x0_images=True)
    assert len(imgs) == len(x0s) == J.E2E["steps"] + 1
    d = dict(final=S.distance(out.cpu(), want),
             img=max(S.distance(a, b) for a, b in zip(imgs[1:], trace["img"])),
             x_start=max(S.distance(a, b) for a, b in zip(x0s[1:], trace["x_start"])))
    _report(test="joint_e2e", precision=precision, **d)
    print("joint end to end", precision, d)
    assert d["final"] <= J.FINAL_BAR and d["img"] <= J.TRAJECTORY_BAR and d["x_start"] <= J.TRAJECTORY_BAR, d


# ------------------------------------------------------------------------------------------------ 4. bit-identities
def test_the_image_in_a_mixed_group_with_another_label_equals_its_solo_run():
    smp = _sampler()
    solo = _e2e(smp, "fp32")
    e = J.E2E
    torch.manual_seed(e["seed"])
    outs = smp.tiled_sample(batch_size=e["batch_size"], condition_x=[J.condition(*e["size"]).cuda(), J.condition(480, 320, 2).cuda()],
                            class_label=torch.tensor([J.LABEL, J.LABEL + 1]).cuda(), num_sample_steps=e["steps"],
                            cond_scale=e["cond_scale"], class_cond_scale=e["class_cond_scale"],
                            guidance_start_steps=e["guidance_start_steps"], class_guidance_start_steps=e["class_guidance_start_steps"],
                            joint_guidance=True, precision="fp32")
    torch.cuda.synchronize()
    assert torch.isfinite(outs[1]).all() and outs[1].shape == (1, 3, 480, 320)
    assert torch.equal(outs[0], solo)
    # the neighbour too, against its own solo run with its own label: passes 0 and 1 read the image's own label row
    torch.manual_seed(e["seed"])
    other = smp.tiled_sample(batch_size=e["batch_size"], condition_x=J.condition(480, 320, 2).cuda(), class_label=_label(J.LABEL + 1),
                             num_sample_steps=e["steps"], cond_scale=e["cond_scale"], class_cond_scale=e["class_cond_scale"],
                             guidance_start_steps=e["guidance_start_steps"], class_guidance_start_steps=e["class_guidance_start_steps"],
                             joint_guidance=True, precision="fp32")
    assert torch.equal(outs[1], other)


def _run300(smp, precision="fp32", steps=4, **over):
    kw = dict(batch_size=9, condition_x=J.condition(300, 300, 3).cuda(), class_label=_label(), num_sample_steps=steps,
              guidance_start_steps=1, precision=precision, **JOINT)
    kw.update(over)
    smp.device_noise_seed = 5
    torch.manual_seed(5)
    out = smp.tiled_sample(**kw)
    torch.cuda.synchronize()
    return out.cpu() if torch.is_tensor(out) else [o.cpu() for o in out]


def test_the_grouping_of_a_joint_step_does_not_change_the_result():
    smp = _sampler()                                        # 9 / 4 tiles: launches of 6 + 3 (the cap of batch_size 9), of 1, of 3
    outs = [_run300(smp, batch_size=bs) for bs in (9, 1, 5)]
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_replayed_graphs_equal_eager_launches_on_device_noise():
    smp = _sampler()
    outs = {}
    try:
        smp.noise_source = "device"
        for mode in ("1", "0"):
            os.environ["SRGD_GRAPHS"] = mode
            smp.model._invalidate_engines()                  # the switch is read at engine creation
            # joint from step 3 on: per parity an eager, a captured and replayed joint steps, after two-pass class-guided ones
            outs[mode] = _run300(smp, "bf16", steps=10, guidance_start_steps=3)
    finally:
        os.environ.pop("SRGD_GRAPHS", None)
        smp.model._invalidate_engines()
        smp.noise_source = "host"
    assert torch.isfinite(outs["1"]).all()
    assert torch.equal(outs["1"], outs["0"])


def test_two_step_lanes_equal_one():
    smp = _sampler()
    keep = smp.step_lanes
    try:
        for noise, prec in (("host", "fp32"), ("device", "bf16")):
            smp.noise_source = noise
            outs = []
            for lanes in (1, 2):
                smp.step_lanes = lanes
                outs.append(_run300(smp, prec, steps=6))
            assert torch.equal(outs[0], outs[1]), (noise, prec)
    finally:
        smp.step_lanes = keep
        smp.noise_source = "host"


@pytest.mark.parametrize("noise", ["host", "device"])
def test_a_seeded_group_equals_the_solo_runs_with_those_seeds(noise):
    smp = _sampler()
    conds = [J.condition(256, 256).cuda(), J.condition(300, 300, 3).cuda(), J.condition(256, 256).cuda()]
    seeds = [11, 12, 13]
    kw = dict(batch_size=6, class_label=_label(), num_sample_steps=3, guidance_start_steps=1, precision="fp32", **JOINT)
    try:
        smp.noise_source = noise
        group = smp.tiled_sample(condition_x=conds, seeds=seeds, **kw)
        for c, s, got in zip(conds, seeds, group):
            smp.device_noise_seed = s
            torch.manual_seed(s)
            assert torch.equal(got, smp.tiled_sample(condition_x=c, **kw)), s
    finally:
        smp.noise_source = "host"
        smp.device_noise_seed = 0
    assert not torch.equal(group[0], group[2])


# ------------------------------------------------------------------------------------------------ 5. existing paths
@pytest.mark.parametrize("scales", [dict(cond_scale=1.5, guidance_start_steps=1), dict(class_cond_scale=2.0, class_guidance_start_steps=1),
                                    dict()], ids=["cond", "class", "none"])
def test_with_one_active_scale_the_keyword_changes_no_byte(scales):
    smp = _sampler()
    outs = []
    for kw in (dict(), dict(joint_guidance=True)):
        torch.manual_seed(9)
        outs.append(smp.tiled_sample(batch_size=4, condition_x=J.condition(300, 300, 3).cuda(), class_label=_label(), num_sample_steps=3,
                                     precision="bf16", with_images=True, with_x0_images=True, **scales, **kw))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1] + outs[0][2], outs[1][1] + outs[1][2]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 6. the C ABI's refusals
def test_the_c_entries_refuse_and_the_run_goes_on():
    from srgd_amd import _lib
    lib = _lib.lib()
    smp = _sampler()
    eng = smp.model.engine("fp32")
    stream = lambda: CT.c_void_p(torch.cuda.current_stream().cuda_stream)
    c01 = J.condition(256, 256).cuda()
    ptr = lambda t: CT.c_void_p(t.data_ptr())

    from srgd_amd.engine import HipEngine

    def joint(e_, img, canvas, s_c, s_l, tiles=False):       # the joint form: passes = 3, the class scale's bits in guidance_kind
        kind = HipEngine._joint_kind(s_l)
        if tiles:
            return lib.srgd_sampler_step_tiles(e_._h, 0, 0, -1, 1, ptr(img), ptr(canvas), None, None, None, 3, kind, s_c, 4, 0, stream())
        return lib.srgd_sampler_step(e_._h, 0, ptr(img), ptr(canvas), None, None, None, 3, kind, s_c, 4, 0, stream())

    # a non-finite scale, then a normal joint step and a normal two-pass step of the same run
    canvas, _, _, _ = _begin(eng, c01, J.LABEL, 4)
    img = torch.randn(1, 3, 256, 256, device="cuda")
    before = img.clone()
    for tiles in (False, True):
        for bad in ((float("nan"), 2.0), (1.5, float("inf")), (float("-inf"), 2.0)):
            assert joint(eng, img, canvas, *bad, tiles=tiles) == -1 and b"finite" in lib.srgd_last_error()
        for one in ((1.0, 2.0), (1.5, 1.0)):                  # a scale of exactly 1: a one- or two-pass step, not a joint one
            assert joint(eng, img, canvas, *one, tiles=tiles) == -1 and b"passes must be 1 or 2" in lib.srgd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(img, before)                          # nothing was launched
    assert joint(eng, img, canvas, 1.5, 2.0) == 0
    eng.sampler_step(1, img, canvas, None, None, None, 2, 1, 2.0, 4)
    torch.cuda.synchronize()
    assert torch.isfinite(img).all() and not torch.equal(img, before)
    # other pass counts are refused as they were
    assert lib.srgd_sampler_step(eng._h, 2, ptr(img), ptr(canvas), None, None, None, 4, 1, 2.0, 4, 0, stream()) == -1
    assert b"passes must be 1 or 2" in lib.srgd_last_error()
    # a run begun without a class
    canvas, _, _, _ = _begin(eng, c01, -1, 4)
    img = before.clone()
    assert joint(eng, img, canvas, 1.5, 2.0) == -1 and b"without a class" in lib.srgd_last_error()
    assert joint(eng, img, canvas, 1.5, 2.0, tiles=True) == -1
    torch.cuda.synchronize()
    assert torch.equal(img, before)
    eng.sampler_step(0, img, canvas, None, None, None, 2, 2, 1.5, 4)
    torch.cuda.synchronize()
    assert torch.isfinite(img).all() and not torch.equal(img, before)
    # no begun run
    out = torch.empty(1, 3, 256, 256, device="cuda")
    eng.sampler_end(img, out)
    assert joint(eng, img, canvas, 1.5, 2.0) == -1 and b"srgd_sampler_begin" in lib.srgd_last_error()
    assert lib.srgd_sampler_step(None, 0, None, None, None, None, None, 3, 3, 1.5, 4, 0, stream()) == -1
    # an EDM run: refused, and the EDM wrapper samples on
    edm = build_edm_sampler(J.DIM)
    good = edm.tiled_sample(batch_size=4, condition_x=c01, class_label=_label(), num_sample_steps=2, precision="fp32")
    e2 = edm.net.engine("fp32")
    from srgd_amd._lib import EdmScalars, SamplerGeometry
    geo = SamplerGeometry(H=256, W=256, Hp=256, Wp=256, left=0, top=0, inner_l=0, inner_t=0, inner_r=256, inner_b=256, tile=256,
                          n_even=1, n_odd=1, n_images=1)
    sc = [EdmScalars(s_noise=1.0, hat_coef=0.0, sigma_hat=1.0, sigma_next=0.5, dt=-0.5, half_dt=-0.25, c_in_hat=1.0, c_skip_hat=0.5,
                     c_out_hat=0.5, c_in_next=1.0, c_skip_next=0.5, c_out_next=0.5, ring_sigma=1.0, clamp=1.0) for _ in range(2)]
    canvas = torch.empty(1, 3, 256, 256, device="cuda")
    e2.edm_begin(geo, c01, canvas, [(0, 0)], [(0, 0)], sc, [0.0] * 4, J.LABEL)
    img = before.clone()
    assert joint(e2, img, canvas, 1.5, 2.0) == -1 and b"srgd_sampler_begin" in lib.srgd_last_error()
    assert joint(e2, img, canvas, 1.5, 2.0, tiles=True) == -1
    work = torch.zeros(2, 3, 256, 256, device="cuda")       # the EDM entries keep one or two passes
    assert lib.srgd_edm_step(e2._h, 0, ptr(img), ptr(canvas), None, ptr(work), None, None, 3, HipEngine._joint_kind(2.0), 1.5, 4, 0,
                             stream()) == -1 and b"passes must be 1 or 2" in lib.srgd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(img, before)
    again = edm.tiled_sample(batch_size=4, condition_x=c01, class_label=_label(), num_sample_steps=2, precision="fp32")
    assert good.shape == again.shape and torch.isfinite(again).all()


# ------------------------------------------------------------------------------------------------ 7. composition
def _psnr(a, b):
    return float(-10.0 * torch.log10(((a.double() - b.double()) ** 2).mean().clamp_min(1e-20)))


def test_joint_guidance_composes_with_the_dynamic_threshold_and_ddim_in_bf16():
    smp = _sampler()
    common = dict(batch_size=9, condition_x=J.condition(300, 300, 3).cuda(), class_label=_label(), num_sample_steps=6)

    def run(precision, **kw):
        torch.manual_seed(21)
        out = smp.tiled_sample(precision=precision, **common, **kw).cpu()
        torch.cuda.synchronize()
        return out
    joint = dict(dynamic_threshold=0.995, sampler="ddim", guidance_start_steps=1, **JOINT)
    parent = dict(class_cond_scale=J.S_L)                    # the parent's class-guided run of the same case
    got = {(p, name): run(p, **kw) for p in ("bf16", "fp32") for name, kw in (("joint", joint), ("class", parent))}
    assert all(torch.isfinite(v).all() for v in got.values())
    psnr_joint, psnr_class = _psnr(got["bf16", "joint"], got["fp32", "joint"]), _psnr(got["bf16", "class"], got["fp32", "class"])
    _report(test="joint_composition", psnr_bf16_vs_fp32_joint=psnr_joint, psnr_bf16_vs_fp32_class_guided=psnr_class)
    print("bf16 against fp32: joint + threshold + ddim", psnr_joint, "dB; class-guided", psnr_class, "dB")
    assert not torch.equal(got["bf16", "joint"], got["bf16", "class"])
    assert psnr_joint >= psnr_class - 3.0, (psnr_joint, psnr_class)
