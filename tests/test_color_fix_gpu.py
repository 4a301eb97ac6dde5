"""``--color_fix``: wavelet / AdaIN colour correction of the sampler's output against its condition, on the GPU
(srgd_image_color_fix / srgd_image_color_fix_images, srgd_amd/csrc/imageio.hip).

Yardstick: tests/color_fix_cases.py - StableSR's two functions restated literally in PyTorch, evaluated in float64.
Tolerances (against the float64 value, worked out from the number formats, not from what the kernels give):
  wavelet  2e-6: 22 fp32 roundings (one for s - c, four per level in the two separable passes, one for c + blur) of values of
           magnitude <= 2: 22 * 2^-24 ~ 1.3e-6.
  adain    2e-6: with float64 statistics and std_s / std_c in [0.5, 2], four fp32 roundings of values of magnitude <= 3 plus the fp32
           rounding of the four statistics: ~ 7e-7.
Everything else here is exact: torch.equal between the batched and the single-image entry, between a group and its solo runs,
between tiled_sample(color_fix=m) and color_fix_on_device on the uncorrected result, and isnan masks equal to the restatement's."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import _lib
from srgd_amd import inference as INF
from srgd_amd.colorfix import scratch_elements
from srgd_amd.synth import synth_state_dict
from tests import color_fix_cases as K
from tests.test_engine_gpu import _schema, build_edm_sampler, build_sampler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"wavelet": 1, "adain": 2}
TOL = 2e-6
GUARD = -7.0


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _single(mode, c, s, in_place=False):
    """srgd_image_color_fix on one [3,h,w] pair; returns the result on the CPU."""
    h, w = c.shape[-2:]
    out, cond = c.cuda().contiguous(), s.cuda().contiguous()
    dst = out if in_place else torch.full_like(out, GUARD)
    scratch = torch.empty(scratch_elements(mode, [0], [(h, w)]), device="cuda")
    rc = _lib.lib().srgd_image_color_fix(_p(out), _p(cond), h, w, MODES[mode], _p(dst), _p(scratch), _stream())
    assert rc == 0, _lib.lib().srgd_last_error()
    torch.cuda.synchronize()
    if not in_place:
        assert torch.equal(out.cpu().view(torch.int32), c.contiguous().view(torch.int32))     # the input is left alone (bitwise: it may hold a NaN)
    return dst.cpu()


def _pairs(mode):
    """The five sizes; for adain both directions of the statistics' ratio (std_s / std_c = 0.5 and 2)."""
    cases = []
    for i, (h, w) in enumerate(K.SIZES):
        c, s = K.pair(h, w, 100 + i, mode)
        cases.append((c, s))
        if mode == "adain":
            cases.append((s, c))
    return cases


# ------------------------------------------------------------------------------------------- 1. the kernel entry
@pytest.mark.parametrize("mode", ["wavelet", "adain"])
def test_single_image_entry_against_the_float64_restatement(mode):
    lo, hi = 0.0, 0.0
    for c, s in _pairs(mode):
        raw = K.literal(mode, c, s)                              # float64, before the clamp
        lo, hi = min(lo, float(raw.min())), max(hi, float(raw.max() - 1))
        want = raw.clamp(0, 1)
        got = _single(mode, c, s)
        err = float((got.double() - want).abs().max())
        print(f"{mode} {tuple(c.shape[-2:])}: max|diff| vs float64 = {err:.3e}, restatement range [{float(raw.min()):.4f}, {float(raw.max()):.4f}]")
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
        assert err <= TOL, (mode, c.shape, err)
    assert lo < 0.0 and hi > 0.0                                 # the restatement leaves [0,1] on these inputs: the clamp is exercised


@pytest.mark.parametrize("mode", ["wavelet", "adain"])
def test_batched_entry_is_bitwise_the_single_image_entry(mode):
    pairs = _pairs(mode)[:5] if mode == "wavelet" else [p for p in _pairs(mode)][::2]
    sizes = [tuple(c.shape[-2:]) for c, _ in pairs]
    assert sizes == K.SIZES
    offsets, off = [], 1                                         # one guard element ahead of and after every image
    for (h, w) in sizes:
        offsets.append(off)
        off += 3 * h * w + 1
    assert any(o % 4 for o in offsets) and len({o % 4 for o in offsets}) > 1
    flat_c = torch.full((off,), GUARD)
    flat_s = torch.full((off,), GUARD)
    for o, (c, s) in zip(offsets, pairs):
        flat_c[o:o + c.numel()] = c.reshape(-1)
        flat_s[o:o + s.numel()] = s.reshape(-1)
    singles = [_single(mode, c, s) for c, s in pairs]
    n = len(sizes)
    offs = (C.c_int64 * n)(*offsets)
    hw = (C.c_int32 * (2 * n))(*[v for sz in sizes for v in sz])
    for in_place in (False, True):
        out, cond = flat_c.cuda(), flat_s.cuda()
        dst = out if in_place else torch.full_like(out, GUARD)
        scratch = torch.empty(scratch_elements(mode, offsets, sizes), device="cuda")
        rc = _lib.lib().srgd_image_color_fix_images(_p(out), _p(cond), offs, hw, n, MODES[mode], _p(dst), _p(scratch), _stream())
        assert rc == 0, _lib.lib().srgd_last_error()
        torch.cuda.synchronize()
        got = dst.cpu()
        for o, (h, w), one in zip(offsets, sizes, singles):
            assert torch.equal(got[o:o + 3 * h * w].view(3, h, w), one), (mode, in_place, (h, w))
            assert float(got[o - 1]) == GUARD and float(got[o + 3 * h * w]) == GUARD, "a neighbour of the image was written"
    for (c, s), one in zip(pairs, singles):                     # the single entry in place too
        assert torch.equal(_single(mode, c, s, in_place=True), one)
    # the Python surface: a list goes through the batched entry, tensors of every accepted rank through it too
    lists = INF.color_fix_on_device([c[None].cuda() for c, _ in pairs], [s[None].cuda() for _, s in pairs], mode)
    for got, one in zip(lists, singles):
        assert got.shape == (1,) + tuple(one.shape) and torch.equal(got[0].cpu(), one)
    c, s = pairs[2]
    assert torch.equal(INF.color_fix_on_device(c.cuda(), s.cuda(), mode).cpu(), singles[2])
    both = INF.color_fix_on_device(torch.stack([c, c]).cuda(), torch.stack([s, s]).cuda(), mode).cpu()
    assert torch.equal(both[0], singles[2]) and torch.equal(both[1], singles[2])


# ------------------------------------------------------------------------------------------- 2. non-finite values
@pytest.mark.parametrize("size", [(33, 64), (256, 256)])
def test_nan_footprint_equals_the_restatement(size):
    h, w = size
    c0, s0 = K.pair(h, w, 7, "wavelet")
    for where in ((1, h // 2, w // 2 + 1), (0, 0, 0), (2, h - 1, w - 1)):      # an interior pixel and two corners
        for target in ("c", "s"):
            c, s = c0.clone(), s0.clone()
            (c if target == "c" else s)[where] = float("nan")
            got = _single("wavelet", c, s)
            want = K.wavelet_literal(c, s)
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (size, where, target)
            assert bool(torch.isnan(got[where])) and not bool(torch.isnan(got[(where[0] + 1) % 3]).any())
            assert 0 < int(torch.isnan(got).sum()) <= 63 * 63
            finite = ~torch.isnan(want)
            assert float((got.double() - want.clamp(0, 1))[finite].abs().max()) <= TOL
            # adain: the channel of the NaN is NaN everywhere, as in the restatement; the other channels are untouched
            ca, sa = K.pair(h, w, 7, "adain")
            (ca if target == "c" else sa)[where] = float("nan")
            got_a, want_a = _single("adain", ca, sa), K.adain_literal(ca, sa)
            assert torch.equal(torch.isnan(got_a), torch.isnan(want_a))
            assert bool(torch.isnan(got_a[where[0]]).all()) and int(torch.isnan(got_a).sum()) == h * w
    c = c0.clone()
    c[1, 5, 9] = float("inf")
    for mode in ("wavelet", "adain"):
        assert not bool(torch.isfinite(_single(mode, c, s0)[1, 5, 9])), mode


# ------------------------------------------------------------------------------------------- 3. C-ABI refusals
def test_cabi_refusals_leave_the_library_usable():
    L = _lib.lib()
    c, s = K.pair(20, 37, 1, "wavelet")
    out, cond = c.cuda(), s.cuda()
    dst = torch.empty_like(out)
    scratch = torch.empty(scratch_elements("wavelet", [0], [(20, 37)]), device="cuda")
    st = _stream()
    offs, hw = (C.c_int64 * 1)(0), (C.c_int32 * 2)(20, 37)

    def err(rc, name):
        assert rc != 0
        msg = L.srgd_last_error().decode()
        assert name in msg, msg
        return msg

    one = "srgd_image_color_fix"
    assert "null" in err(L.srgd_image_color_fix(None, _p(cond), 20, 37, 1, _p(dst), _p(scratch), st), one)
    assert "null" in err(L.srgd_image_color_fix(_p(out), None, 20, 37, 1, _p(dst), _p(scratch), st), one)
    assert "null" in err(L.srgd_image_color_fix(_p(out), _p(cond), 20, 37, 1, None, _p(scratch), st), one)
    assert "null" in err(L.srgd_image_color_fix(_p(out), _p(cond), 20, 37, 1, _p(dst), None, st), one)
    assert "size" in err(L.srgd_image_color_fix(_p(out), _p(cond), 0, 37, 1, _p(dst), _p(scratch), st), one)
    assert "size" in err(L.srgd_image_color_fix(_p(out), _p(cond), 20, -1, 2, _p(dst), _p(scratch), st), one)
    assert "mode" in err(L.srgd_image_color_fix(_p(out), _p(cond), 20, 37, 0, _p(dst), _p(scratch), st), one)
    assert "mode" in err(L.srgd_image_color_fix(_p(out), _p(cond), 20, 37, 3, _p(dst), _p(scratch), st), one)
    many = "srgd_image_color_fix_images"
    assert "n_images" in err(L.srgd_image_color_fix_images(_p(out), _p(cond), offs, hw, 0, 1, _p(dst), _p(scratch), st), many)
    assert "null" in err(L.srgd_image_color_fix_images(_p(out), _p(cond), None, hw, 1, 1, _p(dst), _p(scratch), st), many)
    assert "null" in err(L.srgd_image_color_fix_images(_p(out), _p(cond), offs, None, 1, 1, _p(dst), _p(scratch), st), many)
    assert "mode" in err(L.srgd_image_color_fix_images(_p(out), _p(cond), offs, hw, 1, 7, _p(dst), _p(scratch), st), many)
    assert "size" in err(L.srgd_image_color_fix_images(_p(out), _p(cond), offs, (C.c_int32 * 2)(20, 0), 1, 1, _p(dst), _p(scratch), st), many)
    # ... and a valid call still succeeds
    assert L.srgd_image_color_fix(_p(out), _p(cond), 20, 37, 1, _p(dst), _p(scratch), st) == 0, L.srgd_last_error()
    torch.cuda.synchronize()
    assert float((dst.cpu().double() - K.wavelet_literal(c, s).clamp(0, 1)).abs().max()) <= TOL
    # the Python surface refuses what it cannot pass on
    with pytest.raises(ValueError, match="mode"):
        INF.color_fix_on_device(out, cond, "histogram")
    with pytest.raises(ValueError, match="mode"):
        INF.color_fix_on_device(out, cond, None)
    with pytest.raises(ValueError):
        INF.color_fix_on_device(out, cond[:, :10], "wavelet")
    with pytest.raises(ValueError):
        INF.color_fix_on_device([out[None]], [cond[None], cond[None]], "adain")
    with pytest.raises(ValueError):
        INF.color_fix_on_device([out[None]], cond[None], "adain")
    with pytest.raises(ValueError, match="mode"):
        build_sampler(16).tiled_sample(condition_x=cond[None], color_fix="histogram", num_sample_steps=2)


# ------------------------------------------------------------------------------------------- 4. end to end
E2E_SIZES = [(256, 256), (300, 500), (320, 480)]


def _conds(sizes, seed=21):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in sizes]


def _run(sampler, seed, **kw):
    torch.manual_seed(seed)
    sampler.device_noise_seed = seed
    out = sampler.tiled_sample(**kw)
    return [o.cpu() for o in out] if isinstance(out, (list, tuple)) else out.cpu()


@pytest.mark.parametrize("noise,precision,mode", [("host", "fp32", "wavelet"), ("device", "bf16", "adain"),
                                                  ("device", "f16x3", "wavelet")])
def test_tiled_sample_color_fix_end_to_end(noise, precision, mode):
    sampler = build_sampler(16)
    conds = _conds(E2E_SIZES)
    kw = dict(batch_size=8, num_sample_steps=2, precision=precision)
    labels = [0, 2, 1]
    lab = lambda i: torch.tensor([labels[i]]).cuda()             # noqa: E731
    sampler.noise_source = noise
    try:
        # one image: the keyword is the raw run followed by the public function; None and "none" are today's call
        raw = _run(sampler, 5, condition_x=conds[1], class_label=lab(1), **kw)
        assert torch.equal(_run(sampler, 5, condition_x=conds[1], class_label=lab(1), color_fix=None, **kw), raw)
        assert torch.equal(_run(sampler, 5, condition_x=conds[1], class_label=lab(1), color_fix="none", **kw), raw)
        fixed = _run(sampler, 5, condition_x=conds[1], class_label=lab(1), color_fix=mode, **kw)
        assert torch.equal(fixed, INF.color_fix_on_device(raw.cuda(), conds[1], mode).cpu())
        assert not torch.equal(fixed, raw) and float(fixed.min()) >= 0.0 and float(fixed.max()) <= 1.0
        if mode == "wavelet":               # (the adain bound assumes std_s / std_c in [0.5, 2], which a sampler output need not meet)
            want = K.wavelet_literal(raw[0], conds[1][0].cpu()).clamp(0, 1)
            assert float((fixed[0].double() - want).abs().max()) <= TOL
        # a mixed-size group with per-image labels: per image the solo run with color_fix
        solos = [fixed if i == 1 else _run(sampler, 5, condition_x=conds[i], class_label=lab(i), color_fix=mode, **kw)
                 for i in range(3)]
        group = _run(sampler, 5, condition_x=conds, class_label=torch.tensor(labels).cuda(), color_fix=mode, **kw)
        for i in range(3):
            assert group[i].shape == (1, 3) + E2E_SIZES[i] and torch.equal(group[i], solos[i]), (i, E2E_SIZES[i])
        raw_group = _run(sampler, 5, condition_x=conds, class_label=torch.tensor(labels).cuda(), **kw)
        for a, b in zip(INF.color_fix_on_device([r.cuda() for r in raw_group], conds, mode), group):
            assert torch.equal(a.cpu(), b)
        # ... and with per-image noise seeds (K samples of one image corrected against the same input)
        seeds = [5, 9, 5]
        cs = [conds[1], conds[1], conds[2]]
        seeded = _run(sampler, 123, condition_x=cs, seeds=seeds, class_label=torch.tensor([2, 2, 1]).cuda(), color_fix=mode, **kw)
        assert torch.equal(seeded[0], solos[1]) and torch.equal(seeded[2], solos[2])
        assert torch.equal(seeded[1], _run(sampler, 9, condition_x=conds[1], class_label=lab(1), color_fix=mode, **kw))
        assert not torch.equal(seeded[0], seeded[1])
    finally:
        sampler.noise_source = "host"


def test_batch_tensor_form_trajectories_and_the_edm_wrapper():
    sampler = build_sampler(16)
    g = torch.Generator().manual_seed(3)
    batch = torch.rand(2, 3, 300, 260, generator=g).cuda()
    kw = dict(batch_size=8, num_sample_steps=2, precision="fp32", class_label=torch.tensor([1]).cuda())
    raw = _run(sampler, 4, condition_x=batch, **kw)
    for mode in ("wavelet", "adain"):
        fixed = _run(sampler, 4, condition_x=batch, color_fix=mode, **kw)
        assert fixed.shape == (2, 3, 300, 260)
        assert torch.equal(fixed, INF.color_fix_on_device(raw.cuda(), batch, mode).cpu())
        for b in range(2):
            assert torch.equal(fixed[b:b + 1], _run(sampler, 4, condition_x=batch[b:b + 1], color_fix=mode, **kw))
    # trajectories stay raw: only the returned final image is corrected
    torch.manual_seed(4)
    out_r, imgs_r, x0_r = sampler.tiled_sample(condition_x=batch[:1], with_images=True, with_x0_images=True, **kw)
    torch.manual_seed(4)
    out_f, imgs_f, x0_f = sampler.tiled_sample(condition_x=batch[:1], with_images=True, with_x0_images=True, color_fix="wavelet", **kw)
    assert all(torch.equal(a, b) for a, b in zip(imgs_r, imgs_f)) and all(torch.equal(a, b) for a, b in zip(x0_r, x0_f))
    assert torch.equal(out_f.cpu(), INF.color_fix_on_device(out_r, batch[:1], "wavelet").cpu()) and not torch.equal(out_f, out_r)
    # the EDM wrapper's [B,3,H,W] form
    edm = build_edm_sampler(16)
    ekw = dict(batch_size=8, num_sample_steps=2, precision="bf16", class_label=torch.tensor([0]).cuda())
    raw = _run(edm, 6, condition_x=batch, **ekw)
    assert torch.equal(_run(edm, 6, condition_x=batch, color_fix=None, **ekw), raw)
    for mode in ("wavelet", "adain"):
        fixed = _run(edm, 6, condition_x=batch, color_fix=mode, **ekw)
        assert torch.equal(fixed, INF.color_fix_on_device(raw.cuda(), batch, mode).cpu())
        assert torch.equal(fixed[1:2], _run(edm, 6, condition_x=batch[1:2], color_fix=mode, **ekw))
    assert "color_fix" not in __import__("inspect").signature(sampler.sample).parameters     # un-tiled sample(): out of scope


# ------------------------------------------------------------------------------------------- 5. the command line
def test_cli_color_fix_writes_the_corrected_pngs(tmp_path):
    dim, seed, label = 16, 71, 1
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    indir, outdir = tmp_path / "in", tmp_path / "out"
    indir.mkdir()
    rng = np.random.default_rng(4)
    images = {}
    for name, (h, w) in (("a", (40, 56)), ("b", (64, 48))):
        images[name] = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB")
        images[name].save(indir / f"{name}.png")
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(indir),
           "--output_dir", str(outdir), "--num_sample_steps", "2", "--test_label", str(label), "--batch_size", "4", "--device_noise",
           "--seed", str(seed), "--color_fix", "wavelet", "--lockstep_tiles", "16"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "lock-step group: 2 images" in r.stdout and "color_fix='wavelet'" in r.stdout
    # the un-fixed run in this process, as the driver makes it, then the public function on its tensors
    sampler = build_sampler(dim, weight_seed=3)
    conds = [INF.upsample_bicubic_on_device(images[n], 4, sampler.device) for n in "ab"]
    sampler.noise_source = "device"
    try:
        INF.seed_everything(seed)
        sampler.device_noise_seed = seed
        raw = sampler.tiled_sample(batch_size=4 * 2, condition_x=conds, class_label=torch.LongTensor([label]).cuda(),
                                   num_sample_steps=2, precision="f16x3")
    finally:
        sampler.noise_source = "host"
    fixed = INF.color_fix_on_device(raw, conds, "wavelet")
    for n, f, u in zip("ab", fixed, raw):
        want = INF.unit_tensor_to_u8_on_device(f[0]).cpu().numpy()
        got = np.asarray(Image.open(outdir / f"{n}_out.png").convert("RGB"))
        assert np.array_equal(got, want), n
        assert not np.array_equal(got, INF.unit_tensor_to_u8_on_device(u[0]).cpu().numpy()), n
