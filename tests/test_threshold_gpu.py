"""The dynamic threshold on the MI355X: the library against the numpy restatement of tests/threshold_cases.py as equality of s and of
every byte of both canvases (a NaN is a NaN: sign and payload are not compared), images of a group against their solo calls,
non-finite values, every refusal with real buffers, ``tiled_sample(dynamic_threshold=P)`` against the restated CPU oracle on host noise,
the bitwise invariants of the runs, what is refused, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import _lib
from srgd_amd import inference as INF
from srgd_amd import threshold as TH
from tests import guidance_cases as G
from tests import threshold_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_CANARY = -5.0


def _bits(a):
    """The bit patterns, every NaN as one pattern."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _gpu_step(img, xs, recs, q, weight=TC.WEIGHT):
    """One call on copies of flat numpy buffers -> (img', x_start', s) numpy; the elements of s_out behind the images keep their bytes."""
    d_img, d_xs = (torch.from_numpy(np.array(a)).cuda() for a in (img, xs))
    s = torch.full((len(recs) + 3,), S_CANARY, device="cuda")
    scratch = torch.empty(TH.scratch_bytes(len(recs)), device="cuda", dtype=torch.uint8)
    TH.threshold_step_flat(d_img, d_xs, TH.records(recs), q, weight, s, scratch)
    torch.cuda.synchronize()
    s = s.cpu().numpy()
    assert (s[len(recs):] == S_CANARY).all()
    return d_img.cpu().numpy(), d_xs.cpu().numpy(), s[:len(recs)]


def _outside(recs, size):
    out = np.ones(size, dtype=bool)
    for r in recs:
        TC.update_box(out, r)[...] = False
    return out


# ------------------------------------------------------------------------------------------- the library against the restatement
@pytest.mark.parametrize("name", list(TC.KERNEL_CASES))
def test_the_call_is_the_restatement_bit_for_bit_and_keeps_every_byte_outside_the_update_boxes(name):
    recs, img, xs, q = TC.KERNEL_CASES[name](TH.chunk_elems())
    got_img, got_xs, got_s = _gpu_step(img, xs, recs, q)
    want_img, want_xs = img.copy(), xs.copy()
    want_s = TC.threshold_np(want_img, want_xs, recs, q, TC.WEIGHT)
    assert np.array_equal(_bits(got_s), _bits(want_s)), (got_s[:4], want_s[:4])
    assert np.array_equal(_bits(got_xs), _bits(want_xs)) and np.array_equal(_bits(got_img), _bits(want_img))
    out = _outside(recs, img.size)                       # the canaries, stated on their own: around every box and between the canvases
    assert np.array_equal(got_img[out].view(np.uint32), img[out].view(np.uint32))
    assert np.array_equal(got_xs[out].view(np.uint32), xs[out].view(np.uint32))
    assert out.sum() > 0 and (got_img == TC.SENTINEL).sum() == (img == TC.SENTINEL).sum()
    assert not np.array_equal(_bits(got_xs), _bits(xs))                                   # the call did something


def test_huge_values_outside_the_statistics_box_do_not_move_s_and_are_thresholded():
    recs, img, xs, q = TC.KERNEL_CASES["nested_huge"](TH.chunk_elems())
    _, got_xs, got_s = _gpu_step(img, xs, recs, q)
    calm = xs.copy()
    box = TC.stats_box(xs, recs[0]).copy()
    TC.update_box(calm, recs[0])[...] = 0.25
    TC.stats_box(calm, recs[0])[...] = box
    assert np.array_equal(got_s, _gpu_step(img, calm, recs, q)[2]) and 1.0 < got_s[0] < 1.5
    assert np.abs(xs[~_outside(recs, xs.size)]).max() > 1e30 and np.abs(got_xs[~_outside(recs, xs.size)]).max() == 1.0


def test_zeros_and_denormals_give_s_of_one():
    recs, img, xs, q = TC.case_zeros_and_denormals(TH.chunk_elems())
    box = TC.stats_box(xs, recs[0])
    assert (np.abs(box) < np.float32(1.2e-38)).all() and (box == 0).sum() >= 20 and (box != 0).sum() >= 80
    assert _gpu_step(img, xs, recs, q)[2].tolist() == [1.0] == [float(TC.select_np(box, q)[3])]
    # and the selection itself orders them: with one value above 1 at the top, q = 1 finds it and lower ranks do not
    TC.stats_box(xs, recs[0])[2, 4, 6] = -2.5
    assert _gpu_step(img, xs, recs, 1.0)[2].tolist() == [2.5] and _gpu_step(img, xs, recs, 0.99)[2].tolist() == [1.0]


def test_a_quantile_below_one_is_the_static_clamp_and_leaves_img_alone_where_nothing_changed():
    recs, img, xs, q = TC.KERNEL_CASES["quantile_below_1"](TH.chunk_elems())
    got_img, got_xs, got_s = _gpu_step(img, xs, recs, q)
    assert got_s.tolist() == [1.0]
    inside = ~_outside(recs, xs.size)
    assert np.array_equal(got_xs[inside], np.clip(xs[inside], -1, 1))
    moved = inside & (np.abs(xs) > 1)
    assert moved.sum() > 20 and np.array_equal(got_img[~moved].view(np.uint32), img[~moved].view(np.uint32)) and (got_img[moved] != img[moved]).all()


def test_every_image_of_a_group_is_bit_identical_to_its_solo_call():
    for name in ("three_sizes", "many"):
        recs, img, xs, q = TC.KERNEL_CASES[name](TH.chunk_elems())
        got_img, got_xs, got_s = _gpu_step(img, xs, recs, q)
        assert len(set(got_s.tolist())) > 1
        for k, r in list(enumerate(recs))[::1 if len(recs) < 10 else 43]:
            span = slice(r[0], r[0] + 3 * r[1] * r[2])
            solo_img, solo_xs, solo_s = _gpu_step(img[span], xs[span], [(0,) + tuple(r[1:])], q)        # alone, at offset 0
            assert solo_s[0] == got_s[k] and np.array_equal(_bits(solo_img), _bits(got_img[span])), (name, k)
            assert np.array_equal(_bits(solo_xs), _bits(got_xs[span])), (name, k)


def test_non_finite_values_stay_visible_and_stay_where_they_are():
    chunk = TH.chunk_elems()
    recs, img, xs, q = TC.KERNEL_CASES["one_nan_above"](chunk)           # one NaN above rank hi
    got_img, got_xs, got_s = _gpu_step(img, xs, recs, q)
    assert np.isfinite(got_s).all() and got_s[0] > 1
    assert np.array_equal(np.isnan(got_xs), np.isnan(xs)) and np.isnan(got_xs).sum() == 1
    assert np.array_equal(np.isnan(got_img), np.isnan(got_xs)) and np.isfinite(got_img[~np.isnan(got_img)]).all()
    recs, img, xs, q = TC.KERNEL_CASES["nans_reach_hi"](chunk)           # rank hi is a NaN: the whole update box, nothing else
    got_img, got_xs, got_s = _gpu_step(img, xs, recs, q)
    out = _outside(recs, img.size)
    assert np.isnan(got_s).all() and np.isnan(got_xs[~out]).all() and np.isnan(got_img[~out]).all()
    assert np.array_equal(got_xs[out].view(np.uint32), xs[out].view(np.uint32)) and np.array_equal(got_img[out].view(np.uint32), img[out].view(np.uint32))
    recs, img, xs, q = TC.KERNEL_CASES["inf_at_the_rank"](chunk)         # a_hi = +Inf, frac > 0: s = +Inf
    got_img, got_xs, got_s = _gpu_step(img, xs, recs, q)
    assert np.isposinf(got_s).all()
    ub, was = TC.update_box(got_xs, recs[0]), TC.update_box(xs, recs[0])
    assert np.isnan(ub[np.isinf(was)]).all() and (ub[np.isfinite(was)] == 0).all() and np.isinf(was).sum() == 11


def test_every_refusal_with_real_buffers_launches_nothing_and_writes_nothing():
    recs, img, xs, q = TC.KERNEL_CASES["three_sizes"](TH.chunk_elems())
    d_img, d_xs = torch.from_numpy(img).cuda(), torch.from_numpy(xs).cuda()
    s = torch.full((8,), S_CANARY, device="cuda")
    scratch = torch.full((TH.scratch_bytes(3) + 256,), 77, device="cuda", dtype=torch.uint8)
    arr = TH.records(recs)
    lib = TH.lib()
    ptr = lambda t, off=0: TH.C.c_void_p(t.data_ptr() + off)               # noqa: E731

    def call(**kw):
        a = dict(dict(img=ptr(d_img), xs=ptr(d_xs), recs=arr, n=3, q=q, w=TC.WEIGHT, s=ptr(s), scr=ptr(scratch)), **kw)
        rc = lib.srgd_threshold_step(a["img"], a["xs"], a["recs"], a["n"], a["q"], a["w"], a["s"], a["scr"], None)
        return rc, lib.srgd_threshold_last_error().decode()

    def changed(i, **fields):
        out = (TH.ThresholdImage * 3)()
        for k in range(3):
            for f, _ in TH.ThresholdImage._fields_:
                setattr(out[k], f, fields[f] if k == i and f in fields else getattr(arr[k], f))
        return out
    cases = {"null": [dict(img=None), dict(xs=None), dict(s=None), dict(scr=None), dict(recs=None)],
             "n_images": [dict(n=0), dict(n=-2)],
             "q must be in (0, 1]": [dict(q=0.0), dict(q=1.5), dict(q=float("nan"))],
             "finite": [dict(w=float("nan")), dict(w=float("inf"))],
             "bad size": [dict(recs=changed(2, H=0)), dict(recs=changed(1, W=-1))],
             "bad canvas": [dict(recs=changed(2, Hp=0))],
             "update box": [dict(recs=changed(2, box_h=101)), dict(recs=changed(0, box_l=-1)), dict(recs=changed(1, box_w=81))],
             "statistics box": [dict(recs=changed(0, top=0)), dict(recs=changed(1, W=72)), dict(recs=changed(2, box_l=4, box_w=46))],
             "offset outside": [dict(recs=changed(0, canvas_off=-7))],
             "4-byte aligned": [dict(img=ptr(d_img, 2)), dict(xs=ptr(d_xs, 1)), dict(s=ptr(s, 3))],
             "256-byte aligned": [dict(scr=ptr(scratch, 64))],
             "overlapping canvases": [dict(recs=changed(1, canvas_off=recs[0][0] + 100)), dict(recs=changed(2, canvas_off=recs[1][0]))],
             "overlapping buffers": [dict(xs=ptr(d_img)), dict(xs=ptr(d_img, 4 * 3000)), dict(s=ptr(d_img, 4 * 5000)), dict(img=ptr(d_xs, 8)),
                                     dict(s=ptr(scratch, 512))]}
    for word, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == -1 and word in msg and msg.startswith("srgd_threshold_step: "), (kw, msg)
    torch.cuda.synchronize()
    assert np.array_equal(d_img.cpu().numpy().view(np.uint32), img.view(np.uint32)) and np.array_equal(d_xs.cpu().numpy().view(np.uint32), xs.view(np.uint32))
    assert (s == S_CANARY).all() and (scratch == 77).all()
    with pytest.raises(_lib.SrgdHipError, match="overlapping buffers"):    # through the binding too
        TH.threshold_step_flat(d_img, d_img, arr, q, TC.WEIGHT, s, scratch)
    assert call()[0] == 0                                                  # and the good call goes through
    torch.cuda.synchronize()
    assert (s[:3] > 1).all() and (s[3:] == S_CANARY).all()


# ------------------------------------------------------------------------------------------- end to end against the restated oracle
def _sampler():
    from tests.test_engine_gpu import build_sampler
    sampler = build_sampler(G.DIM)
    sampler.noise_source = "host"
    return sampler


def _run(model, seed, **kw):
    torch.manual_seed(seed)
    model.device_noise_seed = seed
    return model.tiled_sample(**kw)


def _case_kw(name):
    case = TC.E2E_CASES[name]
    base = G.E2E_CASES[case["base"]]
    _, cond = G.e2e_input(case["base"])
    return base, dict(batch_size=base["batch_size"], condition_x=cond.cuda(), class_label=torch.tensor([G.LABEL]).cuda(),
                      num_sample_steps=case["steps"], class_cond_scale=case["class_cond_scale"], **case["kw"])


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", list(TC.E2E_CASES))
def test_the_run_matches_the_restated_oracle(name, precision):
    """Bars: the project's host-noise bars of tests/test_solver_gpu.py - final pixels 1e-3, canvas and predicted-clean-image
    trajectories 2e-3; s relative 2e-3 (it is an element of the x_start trajectory before the division, whose magnitude it has).
    Measured on one MI355X, fp32 / f16x3 (final, canvas, x0, s relative): one 256^2 tile 8.3e-7 / 9.5e-7, 7.6e-6 / 7.6e-6, 2.7e-6 / 3.0e-6,
    2.3e-7 / 2.0e-7; the 300x300 geometry, dpmpp2m logsnr guided 1.8e-6 / 2.3e-6, 1.1e-5 / 1.1e-5, 4.8e-6 / 5.2e-6, 1.4e-6 / 1.9e-6."""
    base, kw = _case_kw(name)
    sampler = _sampler()
    want, trace = TC.e2e_oracle(name)
    log = []
    out, xts, x0s = _run(sampler, base["seed"], precision=precision, with_images=True, with_x0_images=True, dynamic_threshold=TC.P,
                         threshold_log=log, **kw)
    torch.cuda.synchronize()
    steps = TC.E2E_CASES[name]["steps"]
    assert len(xts) == len(x0s) == steps + 1 and out.shape == want.shape
    assert len(log) == 1 and tuple(log[0].shape) == (steps, 1) and log[0].dtype == torch.float32 and log[0].device.type == "cpu"
    err = float((out.cpu() - want).abs().max())
    xt_err = [float((a - b).abs().max()) for a, b in zip(xts[1:], trace["img"])]
    x0_err = [float((a - b).abs().max()) for a, b in zip(x0s[1:], trace["x_start"])]
    s_err = [abs(float(a) / b - 1.0) for a, b in zip(log[0][:, 0], trace["s"])]
    print(f"threshold {name} {precision}: final {err:.3e}, canvas {max(xt_err):.3e}, x0 {max(x0_err):.3e}, s relative {max(s_err):.3e}, "
          f"s {[round(float(v), 4) for v in log[0][:, 0]]}")
    assert trace["s"][0] > 1.0 and float(log[0][0, 0]) > 1.0
    assert err <= 1e-3, err
    assert max(xt_err) <= 2e-3 and max(x0_err) <= 2e-3, (xt_err, x0_err)
    assert max(s_err) <= 2e-3, s_err
    assert not torch.equal(out, _run(sampler, base["seed"], precision=precision, **kw))       # the static clamp gives another image


# ------------------------------------------------------------------------------------------- bitwise
def test_none_and_zero_are_the_call_without_the_keyword():
    _, kw = _case_kw("tile256")
    sampler = _sampler()
    try:
        for source in ("host", "device"):
            sampler.noise_source = source
            plain = _run(sampler, 11, precision="f16x3", **kw)
            for off in (None, 0, 0.0):
                log = []
                assert torch.equal(plain, _run(sampler, 11, precision="f16x3", dynamic_threshold=off, threshold_log=log, **kw)), (source, off)
                assert log == []
            assert not torch.equal(plain, _run(sampler, 11, precision="f16x3", dynamic_threshold=TC.P, **kw)), source
    finally:
        sampler.noise_source = "host"


def test_every_image_of_a_group_is_its_solo_thresholded_run():
    sampler = _sampler()
    g = torch.Generator().manual_seed(9)
    kw = dict(batch_size=8, num_sample_steps=3, precision="bf16", class_label=torch.tensor([1]).cuda(), class_cond_scale=2.0,
              dynamic_threshold=TC.P)
    batch = torch.rand(2, 3, 300, 260, generator=g).cuda()
    log = []
    both = _run(sampler, 4, condition_x=batch, threshold_log=log, **kw)
    assert tuple(log[0].shape) == (3, 2) and (log[0][0] > 1).all()
    for b in range(2):
        solo_log = []
        assert torch.equal(both[b:b + 1], _run(sampler, 4, condition_x=batch[b:b + 1], threshold_log=solo_log, **kw)), b
        assert torch.equal(solo_log[0][:, 0], log[0][:, b])
    # a mixed-size list with seeds, on device noise: K samples of one image among them
    conds = [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in ((256, 256), (300, 500), (96, 132))]
    sampler.noise_source = "device"
    try:
        log = []
        seeded = _run(sampler, 123, condition_x=[conds[1], conds[1], conds[0], conds[2]], seeds=[5, 9, 5, 2], threshold_log=log, **kw)
        assert tuple(log[0].shape) == (3, 4)
        for k, (c, s, got) in enumerate(zip((conds[1], conds[1], conds[0], conds[2]), (5, 9, 5, 2), seeded)):
            solo_log = []
            assert torch.equal(got, _run(sampler, s, condition_x=c, threshold_log=solo_log, **kw)), s
            assert torch.equal(solo_log[0][:, 0], log[0][:, k])
        assert not torch.equal(seeded[0], seeded[1])
    finally:
        sampler.noise_source = "host"


def test_a_late_start_thresholds_the_executed_steps_only():
    _, kw = _case_kw("tile256")
    sampler = _sampler()
    log = []
    out = _run(sampler, 3, precision="f16x3", generation_start_steps=2, dynamic_threshold=TC.P, threshold_log=log, **kw)
    assert tuple(log[0].shape) == (kw["num_sample_steps"] - 2, 1) and torch.isfinite(out).all() and (log[0] >= 1).all()


def test_a_sharded_canvas_and_the_edm_wrapper_refuse_the_percentile():
    from tests.test_engine_gpu import build_edm_sampler
    _, kw = _case_kw("tile256")
    sampler = _sampler()
    sampler.canvas_group = object()
    try:
        with pytest.raises(NotImplementedError, match="canvas_group"):
            _run(sampler, 3, dynamic_threshold=TC.P, **kw)
    finally:
        sampler.canvas_group = None
    edm = build_edm_sampler(G.DIM)
    with pytest.raises(NotImplementedError, match="DDPM sampler only"):
        edm.tiled_sample(condition_x=kw["condition_x"], class_label=kw["class_label"], batch_size=4, num_sample_steps=2, dynamic_threshold=TC.P)


# ------------------------------------------------------------------------------------------- the command line
def test_cli_dynamic_threshold_writes_what_the_python_call_produces_and_zero_is_the_plain_run(tmp_path):
    from srgd_amd.config import load_config
    from srgd_amd.synth import synth_state_dict
    from tests.test_engine_gpu import _schema
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    indir = tmp_path / "in"
    indir.mkdir()
    Image.fromarray(G.smooth_lr(24, 40, 4), "RGB").save(indir / "a.png")
    base = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(indir),
            "--num_sample_steps", "3", "--test_label", "1", "--batch_size", "4", "--device_noise", "--seed", "71", "--class_cond_scale", "2.0"]
    first = subprocess.run(base + ["--output_dir", str(tmp_path / "on"), "--dynamic_threshold", "0.995"], cwd=ROOT, capture_output=True,
                           text=True, timeout=300)
    assert first.returncode == 0, first.stderr[-3000:]           # one child at a time
    second = subprocess.run(base + ["--output_dir", str(tmp_path / "zero"), "--dynamic_threshold", "0"], cwd=ROOT, capture_output=True,
                            text=True, timeout=300)
    assert second.returncode == 0, second.stderr[-3000:]
    assert os.listdir(tmp_path / "on") == os.listdir(tmp_path / "zero") == ["a_out.png"]
    # the Python calls on the model the command line builds
    import logging
    cfg = load_config(str(conf))
    cfg.num_sample_steps, cfg.ckpt_path = 3, str(ckpt)
    model = INF.get_model(cfg, logging.getLogger("test")).module.eval().to(torch.device("cuda", torch.cuda.current_device()))
    model.noise_source, model.precision = "device", INF.parse_args(["-c", str(conf), "-m", str(ckpt), "--input_dir", "i", "--output_dir", "o"]).precision
    image = Image.open(indir / "a.png").convert("RGB")
    kw = dict(batch_size=4, test_label=1, class_cond_scale=2.0, num_sample_steps=3, seed=71)
    with_flag = INF.sr_target_image(image, model, dynamic_threshold=0.995, **kw)
    plain = INF.sr_target_image(image, model, **kw)
    on, zero = (np.asarray(Image.open(tmp_path / d / "a_out.png").convert("RGB")) for d in ("on", "zero"))
    assert on.shape == (96, 160, 3) and np.array_equal(on, np.asarray(with_flag)) and np.array_equal(zero, np.asarray(plain))
    assert not np.array_equal(on, zero)
