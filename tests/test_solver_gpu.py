"""The few-step samplers on the MI355X: the history kernel against numpy fp32 as equality (tests/solver_cases.py (c)) with every byte
outside the boxes kept, non-finite values, ``tiled_sample(sampler=..., step_spacing=...)`` against the restated CPU oracle (d) on host
noise, the bitwise invariants of the runs, ddim with eta = 1 against the default run, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import model as MODEL
from srgd_amd import solver as SV
from tests import guidance_cases as G
from tests import solver_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gpu_step(img, xs, xp, recs, w):
    """One call on copies of flat numpy buffers -> (img', x_start', x_prev') numpy."""
    d = [torch.from_numpy(np.array(a)).cuda() for a in (img, xs, xp)]
    SV.history_step_flat(d[0], d[1], d[2], SV.records(recs), w)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in d]


# ------------------------------------------------------------------------------------------- (e) the kernel against numpy fp32
@pytest.mark.parametrize("w", SC.KERNEL_WEIGHTS)
@pytest.mark.parametrize("group", list(SC.KERNEL_GROUPS))
def test_the_history_step_is_numpy_fp32_bit_for_bit_and_keeps_every_byte_outside_the_boxes(group, w):
    recs = SC.KERNEL_GROUPS[group]
    img, xs, xp = SC.kernel_buffers(recs, 3)
    got_img, got_xs, got_xp = _gpu_step(img, xs, xp, recs, w)
    want_img, want_xp = img.copy(), xp.copy()
    SC.history_np(want_img, xs, want_xp, recs, w)
    assert np.array_equal(_bits(got_img), _bits(want_img)) and np.array_equal(_bits(got_xp), _bits(want_xp))
    assert np.array_equal(_bits(got_xs), _bits(xs))
    assert not np.array_equal(want_img, img) and not np.array_equal(want_xp, xp)          # the boxes did change
    inside = np.zeros(img.size, dtype=bool)              # the canaries, stated on their own: around every box and between the canvases
    for (off, hp, wp, top, left, h, wd) in recs:
        inside[off:off + 3 * hp * wp].reshape(3, hp, wp)[:, top:top + h, left:left + wd] = True
    assert np.array_equal(_bits(got_img)[~inside], _bits(img)[~inside]) and np.array_equal(_bits(got_xp)[~inside], _bits(xp)[~inside])
    assert (~inside).sum() > 0 and (got_img == SC.SENTINEL).sum() == (img == SC.SENTINEL).sum()


def test_an_image_of_a_group_is_bit_identical_to_its_solo_call():
    recs = SC.KERNEL_GROUPS["group"]
    img, xs, xp = SC.kernel_buffers(recs, 5)
    got_img, _, got_xp = _gpu_step(img, xs, xp, recs, 0.37)
    for (off, hp, wp, top, left, h, wd) in recs:         # alone, at offset 0 (the last one: the four-dword form in both calls)
        span = slice(off, off + 3 * hp * wp)
        solo_img, _, solo_xp = _gpu_step(img[span], xs[span], xp[span], [(0, hp, wp, top, left, h, wd)], 0.37)
        assert np.array_equal(_bits(got_img[span]), _bits(solo_img)) and np.array_equal(_bits(got_xp[span]), _bits(solo_xp))
    # the same canvas one element further on: the dword form gives the same bytes as the four-dword form
    off, hp, wp, top, left, h, wd = recs[2]
    span = slice(off, off + 3 * hp * wp)
    pad = lambda a: np.concatenate([np.zeros(1, np.float32), a[span]])       # noqa: E731
    moved_img, _, moved_xp = _gpu_step(pad(img), pad(xs), pad(xp), [(1, hp, wp, top, left, h, wd)], 0.37)
    assert np.array_equal(_bits(moved_img[1:]), _bits(got_img[span])) and np.array_equal(_bits(moved_xp[1:]), _bits(got_xp[span]))


def test_a_weight_of_zero_leaves_img_alone_even_where_the_history_is_nan():
    recs = SC.KERNEL_GROUPS["group"]
    img, xs, xp = SC.kernel_buffers(recs, 7)
    for (off, hp, wp, top, left, h, wd) in recs:
        xp[off:off + 3 * hp * wp].reshape(3, hp, wp)[1, top + 2, left:left + wd] = np.nan
    got_img, got_xs, got_xp = _gpu_step(img, xs, xp, recs, 0.0)
    assert np.array_equal(_bits(got_img), _bits(img)) and np.array_equal(_bits(got_xs), _bits(xs))
    want_xp = xp.copy()
    SC.history_np(img.copy(), xs, want_xp, recs, 0.0)
    assert np.array_equal(_bits(got_xp), _bits(want_xp)) and np.isfinite(got_xp[got_xp != SC.SENTINEL]).all()


def test_nan_and_inf_in_x_start_stay_visible_and_stay_where_they_are():
    recs = SC.KERNEL_GROUPS["group"]
    img, xs, xp = SC.kernel_buffers(recs, 9)
    planted = np.zeros(img.size, dtype=bool)
    for k, (off, hp, wp, top, left, h, wd) in enumerate(recs):
        for c, y, x, v in ((0, 0, 0, np.nan), (1, h - 1, wd - 1, np.inf), (2, h // 2, wd // 2 + k, -np.inf)):
            at = off + (c * hp + top + y) * wp + left + x
            xs[at], planted[at] = v, True
    got_img, _, got_xp = _gpu_step(img, xs, xp, recs, -1.25)
    want_img, want_xp = img.copy(), xp.copy()
    SC.history_np(want_img, xs, want_xp, recs, -1.25)
    for got, want in ((got_img, want_img), (got_xp, want_xp)):
        assert np.array_equal(~np.isfinite(got), planted)
        assert np.array_equal(_bits(got[~planted]), _bits(want[~planted]))
    assert np.isnan(got_img[planted]).sum() == len(recs) and np.isinf(got_img[planted]).sum() == 2 * len(recs)


# ------------------------------------------------------------------------------------------- (f) end to end against yardstick (d)
def _sampler():
    from tests.test_engine_gpu import build_sampler
    sampler = build_sampler(G.DIM)
    sampler.noise_source = "host"
    return sampler


def _run(model, seed, **kw):
    torch.manual_seed(seed)
    model.device_noise_seed = seed
    return model.tiled_sample(**kw)


def _base_kw(base):
    case = G.E2E_CASES[base]
    _, cond = G.e2e_input(base)
    return case, dict(batch_size=case["batch_size"], condition_x=cond.cuda(), class_label=torch.tensor([G.LABEL]).cuda(),
                      num_sample_steps=case["steps"], class_cond_scale=case["class_cond_scale"])


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", list(SC.E2E_CASES))
def test_the_run_matches_the_restated_oracle(name, precision):
    """Bars: the project's host-noise bars - final pixels 1e-3, canvas and predicted-clean-image trajectories 2e-3.
    Measured on one MI355X, fp32 / f16x3 (final, canvas, x0): ddim eta 0 7.5e-5 / 5.7e-5, 1.5e-4 / 1.8e-4, 2.3e-4 / 2.3e-4; ddim eta 0.5
    2.2e-5 / 1.9e-5, 4.5e-5 / 3.9e-5, 2.3e-4 / 2.3e-4; dpmpp2m logsnr 6.7e-5 / 7.4e-5, 1.3e-4 / 1.5e-4, 2.3e-4 / 2.3e-4; the 300x300
    geometry, dpmpp2m logsnr guided 1.6e-4 / 1.5e-4, 5.6e-4 / 4.7e-4, 5.5e-4 / 5.6e-4."""
    case, kw = _base_kw(SC.E2E_CASES[name]["base"])
    sampler = _sampler()
    want, trace = SC.e2e_oracle(name)
    out, xts, x0s = _run(sampler, case["seed"], precision=precision, with_images=True, with_x0_images=True, **kw, **SC.sampler_kw(name))
    torch.cuda.synchronize()
    assert len(xts) == len(x0s) == case["steps"] + 1 and out.shape == want.shape
    err = float((out.cpu() - want).abs().max())
    xt_err = [float((a - b).abs().max()) for a, b in zip(xts[1:], trace["img"])]
    x0_err = [float((a - b).abs().max()) for a, b in zip(x0s[1:], trace["x_start"])]
    print(f"solver {name} {precision}: final {err:.3e}, canvas {max(xt_err):.3e}, x0 {max(x0_err):.3e}")
    assert err <= 1e-3, err
    assert max(xt_err) <= 2e-3 and max(x0_err) <= 2e-3, (xt_err, x0_err)
    assert not torch.equal(out, _run(sampler, case["seed"], precision=precision, **kw))      # it is another sampler


# ------------------------------------------------------------------------------------------- (g) equalities
def test_the_explicit_defaults_are_the_call_without_the_keywords():
    case, kw = _base_kw("tile256")
    sampler = _sampler()
    try:
        for source in ("host", "device"):
            sampler.noise_source = source
            plain = _run(sampler, 11, precision="f16x3", **kw)
            explicit = _run(sampler, 11, precision="f16x3", sampler="ddpm", eta=None, step_spacing="time", **kw)
            assert torch.equal(plain, explicit), source
            assert not torch.equal(plain, _run(sampler, 11, precision="f16x3", step_spacing="logsnr", **kw)), source
    finally:
        sampler.noise_source = "host"


def test_every_image_of_a_group_is_its_solo_dpmpp2m_run():
    sampler = _sampler()
    g = torch.Generator().manual_seed(9)
    solver = dict(sampler="dpmpp2m", step_spacing="logsnr")
    kw = dict(batch_size=8, num_sample_steps=4, precision="bf16", class_label=torch.tensor([1]).cuda())
    batch = torch.rand(2, 3, 300, 260, generator=g).cuda()
    both = _run(sampler, 4, condition_x=batch, **kw, **solver)
    for b in range(2):
        assert torch.equal(both[b:b + 1], _run(sampler, 4, condition_x=batch[b:b + 1], **kw, **solver)), b
    assert not torch.equal(both, _run(sampler, 4, condition_x=batch, **kw, sampler="ddim", step_spacing="logsnr"))   # the history counts
    # a mixed-size list with seeds, on device noise: K samples of one image among them
    conds = [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in ((256, 256), (300, 500), (96, 132))]
    sampler.noise_source = "device"
    try:
        seeded = _run(sampler, 123, condition_x=[conds[1], conds[1], conds[0], conds[2]], seeds=[5, 9, 5, 2], **kw, **solver)
        for c, s, got in zip((conds[1], conds[1], conds[0], conds[2]), (5, 9, 5, 2), seeded):
            assert torch.equal(got, _run(sampler, s, condition_x=c, **kw, **solver)), s
        assert not torch.equal(seeded[0], seeded[1])
    finally:
        sampler.noise_source = "host"


def test_a_late_start_launches_its_first_step_with_a_weight_of_zero(monkeypatch):
    case, kw = _base_kw("tile256")
    sampler = _sampler()
    seen = []
    real = MODEL.history_step_flat

    def spy(img, x_start, x_prev, recs, w):
        seen.append(w)
        return real(img, x_start, x_prev, recs, w)
    monkeypatch.setattr(MODEL, "history_step_flat", spy)
    out = _run(sampler, 3, precision="f16x3", generation_start_steps=2, sampler="dpmpp2m", step_spacing="logsnr", **kw)
    want = SV.history_weights(MODEL._log_snr_levels(case["steps"], "logsnr"), 2)[2:]
    assert seen == want and len(seen) == case["steps"] - 2 and seen[0] == 0.0 and seen[-1] == 0.0 and all(w > 0 for w in seen[1:-1])
    assert torch.isfinite(out).all()
    # with every weight at zero the run is ddim at eta = 0 byte for byte: the history call alone changes nothing
    monkeypatch.setattr(MODEL, "history_step_flat", lambda img, x_start, x_prev, recs, w: real(img, x_start, x_prev, recs, 0.0))
    flat = _run(sampler, 3, precision="f16x3", generation_start_steps=2, sampler="dpmpp2m", step_spacing="logsnr", **kw)
    monkeypatch.setattr(MODEL, "history_step_flat", real)
    ddim = _run(sampler, 3, precision="f16x3", generation_start_steps=2, sampler="ddim", eta=0.0, step_spacing="logsnr", **kw)
    assert torch.equal(flat, ddim) and not torch.equal(out, ddim)


# ------------------------------------------------------------------------------------------- (h) closeness
def test_ddim_with_eta_one_is_the_default_run_within_the_final_bar():
    """Measured on one MI355X: 1.1e-5 (fp32 engine) - the tables agree within an fp32 rounding, the draws are the same."""
    case, kw = _base_kw("tile256")
    sampler = _sampler()
    plain = _run(sampler, case["seed"], precision="fp32", **kw)
    ddim = _run(sampler, case["seed"], precision="fp32", sampler="ddim", eta=1.0, **kw)
    err = float((plain - ddim).abs().max())
    print(f"ddim eta = 1 against the default run, tile256 fp32: max|diff| = {err:.3e}")
    assert err <= 1e-3, err


# ------------------------------------------------------------------------------------------- (i) the command line
def test_cli_sampler_flags_write_a_file(tmp_path):
    from srgd_amd.synth import synth_state_dict
    from tests.test_engine_gpu import _schema
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    indir, outdir = tmp_path / "in", tmp_path / "out"
    indir.mkdir()
    Image.fromarray(G.smooth_lr(24, 40, 4), "RGB").save(indir / "a.png")
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(indir),
           "--output_dir", str(outdir), "--num_sample_steps", "4", "--test_label", "1", "--batch_size", "4", "--device_noise", "--seed",
           "71", "--sampler", "ddim", "--eta", "0.5", "--step_spacing", "logsnr"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:]
    assert os.listdir(outdir) == ["a_out.png"]
    assert Image.open(outdir / "a_out.png").size == (160, 96)
