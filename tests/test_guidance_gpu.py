"""LR-consistency guidance on the MI355X: the two kernels against the float64 yardstick (tests/guidance_cases.py (a)) with every byte
outside the crop box kept, a group against its solo calls, the footprint of a NaN, ``tiled_sample(consistency_guidance=...)`` against
the guided CPU oracle (yardstick (b)) on host noise, the bitwise invariants of the guided run, and the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import guidance as GD
from tests import consistency_cases as K
from tests import guidance_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                 # a copy: the cases are read-only


def _solo(h, w, weights, x_start=None):
    """One call on the kernel case of an LR size -> (img', x_start') numpy [3,Hp,Wp]."""
    img, xs, cond, (hp, wp, top, left) = G.kernel_case(h, w)
    d_img, d_xs, d_cond = _dev(img).view(-1), _dev(xs if x_start is None else x_start).view(-1), _dev(cond).view(-1)
    recs, low = GD.records([(0, 0, hp, wp, top, left, 4 * h, 4 * w)])
    scratch = torch.empty(GD.scratch_bytes(low), device="cuda", dtype=torch.uint8)
    GD.guide_step_flat(d_img, d_xs, d_cond, recs, weights[0], weights[1], scratch)
    torch.cuda.synchronize()
    return d_img.view(3, hp, wp).cpu().numpy(), d_xs.view(3, hp, wp).cpu().numpy()


# ------------------------------------------------------------------------------------------- 1. the kernels against yardstick (a)
@pytest.mark.parametrize("weights", G.WEIGHTS, ids=lambda v: f"w{v[0]}_{v[1]}")
@pytest.mark.parametrize("h,w", G.KERNEL_SIZES)
def test_the_step_matches_the_float64_yardstick_and_keeps_every_byte_outside_the_crop_box(h, w, weights):
    img, xs, cond, (hp, wp, top, left) = G.kernel_case(h, w)
    got_img, got_xs = _solo(h, w, weights)
    want_img, want_xs = G.guide64(img, xs, cond, top, left, *weights)
    box = (slice(None), slice(top, top + 4 * h), slice(left, left + 4 * w))
    err = max(float(np.abs(got_img[box] - want_img[box]).max()), float(np.abs(got_xs[box] - want_xs[box]).max()))
    print(f"guidance step {h}x{w} weights {weights}: max|gpu - float64| = {err:.3e} (bar {G.KERNEL_BAR:.3e})")
    assert err <= G.KERNEL_BAR, err
    outside = np.ones((3, hp, wp), dtype=bool)
    outside[box] = False
    for got, src in ((got_img, img), (got_xs, xs)):
        assert np.array_equal(got[outside].view(np.uint32), src[outside].view(np.uint32))
        assert (src[outside] == G.SENTINEL).all() and not np.array_equal(got[box], src[box])


# ------------------------------------------------------------------------------------------- 2. a group and its solo calls
def test_a_group_at_odd_offsets_is_bit_identical_to_its_solo_calls():
    weights = G.WEIGHTS[0]
    gaps = (3, 5, 7)                                       # elements in front of every image's canvas / condition
    images, canv_parts, xs_parts, cond_parts, canvas_off, cond_off = [], [], [], [], 0, 0
    for (h, w), gap in zip(G.KERNEL_SIZES, gaps):
        img, xs, cond, (hp, wp, top, left) = G.kernel_case(h, w)
        canvas_off += gap
        cond_off += gap + 1
        images.append((canvas_off, cond_off, hp, wp, top, left, 4 * h, 4 * w))
        canv_parts += [np.full(gap, G.SENTINEL, np.float32), img.ravel()]
        xs_parts += [np.full(gap, G.SENTINEL, np.float32), xs.ravel()]
        cond_parts += [np.full(gap + 1, G.SENTINEL, np.float32), cond.ravel()]
        canvas_off += img.size
        cond_off += cond.size
    d_img, d_xs, d_cond = _dev(np.concatenate(canv_parts)), _dev(np.concatenate(xs_parts)), _dev(np.concatenate(cond_parts))
    recs, low = GD.records(images)
    scratch = torch.empty(GD.scratch_bytes(low), device="cuda", dtype=torch.uint8)
    GD.guide_step_flat(d_img, d_xs, d_cond, recs, weights[0], weights[1], scratch)
    torch.cuda.synchronize()
    got_img, got_xs = d_img.cpu().numpy(), d_xs.cpu().numpy()
    covered = np.zeros(got_img.size, dtype=bool)
    for (h, w), m in zip(G.KERNEL_SIZES, images):
        solo_img, solo_xs = _solo(h, w, weights)
        span = slice(m[0], m[0] + solo_img.size)
        covered[span] = True
        assert np.array_equal(got_img[span].view(np.uint32), solo_img.ravel().view(np.uint32)), (h, w)
        assert np.array_equal(got_xs[span].view(np.uint32), solo_xs.ravel().view(np.uint32)), (h, w)
    assert (got_img[~covered] == G.SENTINEL).all() and (got_xs[~covered] == G.SENTINEL).all() and (~covered).sum() == sum(gaps)


# ------------------------------------------------------------------------------------------- 3. non-finite values
@pytest.mark.parametrize("where", ["interior", "corner"])
def test_a_nan_stays_visible_and_spreads_no_farther_than_the_windows(where):
    h, w = 16, 23
    weights = G.WEIGHTS[0]
    img, xs, cond, (hp, wp, top, left) = G.kernel_case(h, w)
    py, px = (33, 41) if where == "interior" else (4 * h - 1, 0)
    bad = xs.copy()
    bad[1, top + py, left + px] = np.nan
    clean_img, clean_xs = _solo(h, w, weights)
    got_img, got_xs = _solo(h, w, weights, x_start=bad)
    assert np.isnan(got_img[1, top + py, left + px]) and np.isnan(got_xs[1, top + py, left + px])
    yy, xx = np.mgrid[0:hp, 0:wp]
    far = np.maximum(np.abs(yy - (top + py)), np.abs(xx - (left + px))) > 24
    for c in range(3):
        keep = far if c == 1 else np.ones_like(far)      # the other planes never see it
        assert np.array_equal(got_img[c][keep].view(np.uint32), clean_img[c][keep].view(np.uint32)), c
        assert np.array_equal(got_xs[c][keep].view(np.uint32), clean_xs[c][keep].view(np.uint32)), c
    assert np.isnan(got_img[1]).sum() > 1                  # it does reach its neighbours


# ------------------------------------------------------------------------------------------- 4. end to end against yardstick (b)
def _sampler():
    from tests.test_engine_gpu import build_sampler
    sampler = build_sampler(G.DIM)
    sampler.noise_source = "host"
    return sampler


def _run(sampler, seed, **kw):
    torch.manual_seed(seed)
    sampler.device_noise_seed = seed
    return sampler.tiled_sample(**kw)


def _case_kw(name):
    case = G.E2E_CASES[name]
    lr, cond = G.e2e_input(name)
    kw = dict(batch_size=case["batch_size"], condition_x=cond.cuda(), class_label=torch.tensor([G.LABEL]).cuda(),
              num_sample_steps=case["steps"], class_cond_scale=case["class_cond_scale"])
    guide = dict(consistency_guidance=case["weight"], consistency_guidance_start_steps=case["start"])
    return case, lr, kw, guide


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", list(G.E2E_CASES))
def test_the_guided_run_matches_the_guided_oracle(name, precision):
    """Bars: the project's host-noise bars - final pixels 1e-3, canvas and predicted-clean-image trajectories 2e-3."""
    case, lr, kw, guide = _case_kw(name)
    sampler = _sampler()
    want, trace = G.e2e_oracle(name, True)
    out, xts, x0s = _run(sampler, case["seed"], precision=precision, with_images=True, with_x0_images=True, **kw, **guide)
    torch.cuda.synchronize()
    assert len(xts) == len(x0s) == case["steps"] + 1 and out.shape == want.shape
    err = float((out.cpu() - want).abs().max())
    xt_err = [float((a - b).abs().max()) for a, b in zip(xts[1:], trace["img"])]
    x0_err = [float((a - b).abs().max()) for a, b in zip(x0s[1:], trace["x_start"])]
    plain = _run(sampler, case["seed"], precision=precision, **kw)
    mse, mse_plain = G.lr_mse(out, lr), G.lr_mse(plain, lr)
    print(f"guided {name} {precision}: final {err:.3e}, canvas {max(xt_err):.3e}, x0 {max(x0_err):.3e}; "
          f"LR-MSE guided {mse:.2f}, unguided {mse_plain:.2f}")
    assert err <= 1e-3, err
    assert max(xt_err) <= 2e-3 and max(x0_err) <= 2e-3, (xt_err, x0_err)
    assert mse < mse_plain, (mse, mse_plain)
    assert not torch.equal(out, plain)


# ------------------------------------------------------------------------------------------- 5. invariants
def test_a_run_guided_from_past_its_last_step_is_the_unguided_run():
    case, lr, kw, guide = _case_kw("tile256")
    sampler = _sampler()
    plain = _run(sampler, 3, precision="f16x3", **kw)
    late = _run(sampler, 3, precision="f16x3", **kw, consistency_guidance=1.0, consistency_guidance_start_steps=case["steps"])
    zero = _run(sampler, 3, precision="f16x3", **kw, consistency_guidance=0.0)
    assert torch.equal(late, plain) and torch.equal(zero, plain)
    last = _run(sampler, 3, precision="f16x3", **kw, consistency_guidance=1.0, consistency_guidance_start_steps=case["steps"] - 1)
    assert not torch.equal(last, plain)                    # the last step is guided too


def test_every_image_of_a_group_is_its_solo_guided_run():
    sampler = _sampler()
    g = torch.Generator().manual_seed(9)
    guide = dict(consistency_guidance=0.75, consistency_guidance_start_steps=1)
    kw = dict(batch_size=8, num_sample_steps=3, precision="bf16", class_label=torch.tensor([1]).cuda())
    # [B,3,H,W]
    batch = torch.rand(2, 3, 300, 260, generator=g).cuda()
    both = _run(sampler, 4, condition_x=batch, **kw, **guide)
    for b in range(2):
        assert torch.equal(both[b:b + 1], _run(sampler, 4, condition_x=batch[b:b + 1], **kw, **guide)), b
    assert not torch.equal(both, _run(sampler, 4, condition_x=batch, **kw))
    # a mixed-size list
    conds = [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in ((256, 256), (300, 500), (96, 132))]
    mixed = _run(sampler, 5, condition_x=conds, **kw, **guide)
    for c, got in zip(conds, mixed):
        assert torch.equal(got, _run(sampler, 5, condition_x=c, **kw, **guide)), tuple(c.shape)
    # a seeded group on device noise: K samples of one image
    sampler.noise_source = "device"
    try:
        seeded = _run(sampler, 123, condition_x=[conds[1], conds[1], conds[0]], seeds=[5, 9, 5], **kw, **guide)
        for c, s, got in zip((conds[1], conds[1], conds[0]), (5, 9, 5), seeded):
            assert torch.equal(got, _run(sampler, s, condition_x=c, **kw, **guide)), s
        assert not torch.equal(seeded[0], seeded[1])
    finally:
        sampler.noise_source = "host"


def test_two_step_lanes_are_bit_identical_to_one_and_bf16_lowers_lr_mse():
    case, lr, kw, guide = _case_kw("geo300")
    sampler = _sampler()
    saved = sampler.step_lanes
    try:
        outs = {}
        for lanes in (1, 2):
            sampler.step_lanes = lanes
            outs[lanes] = _run(sampler, case["seed"], precision="bf16", **kw, **guide)
        plain = _run(sampler, case["seed"], precision="bf16", **kw)
    finally:
        sampler.step_lanes = saved
    assert torch.equal(outs[1], outs[2])
    assert torch.isfinite(outs[1]).all() and float(outs[1].min()) >= 0 and float(outs[1].max()) <= 1
    mse, mse_plain = G.lr_mse(outs[1], lr), G.lr_mse(plain, lr)
    print(f"guided geo300 bf16: LR-MSE guided {mse:.2f}, unguided {mse_plain:.2f}")
    assert mse < mse_plain, (mse, mse_plain)


# ------------------------------------------------------------------------------------------- 6. the command line
def test_cli_consistency_guidance_raises_the_lr_psnr(tmp_path):
    from srgd_amd.synth import synth_state_dict
    from tests.test_engine_gpu import _schema
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    indir, outdir, plain = tmp_path / "in", tmp_path / "out", tmp_path / "plain"
    indir.mkdir()
    lrs = {"a.png": G.smooth_lr(40, 56, 4), "b.png": G.smooth_lr(24, 24, 5)}
    for name, lr in lrs.items():
        Image.fromarray(lr, "RGB").save(indir / name)
    base = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(indir),
            "--num_sample_steps", "3", "--test_label", "1", "--batch_size", "4", "--device_noise", "--seed", "71", "--consistency"]
    first = subprocess.run(base + ["--output_dir", str(plain)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert first.returncode == 0, first.stderr[-3000:]           # one child at a time
    second = subprocess.run(base + ["--output_dir", str(outdir), "--consistency_guidance", "1"], cwd=ROOT, capture_output=True,
                            text=True, timeout=300)
    assert second.returncode == 0, second.stderr[-3000:]         # only after the first returned 0
    names = ["a_out.png", "b_out.png"]
    assert sorted(os.listdir(outdir)) == sorted(os.listdir(plain)) == sorted(names + ["consistency.json"])
    doc, doc_plain = json.load(open(outdir / "consistency.json")), json.load(open(plain / "consistency.json"))
    for n, lr in zip(names, lrs.values()):
        assert doc["files"][n] == K.yardstick(np.asarray(Image.open(outdir / n).convert("RGB")), lr)[2]
        assert doc["files"][n]["lr_psnr"] > doc_plain["files"][n]["lr_psnr"], n
    assert doc["mean"]["lr_psnr"] > doc_plain["mean"]["lr_psnr"]
