"""Per-image class labels on the GPU: ``ConditionalSRUnet.forward`` with a ``[B]`` label, and lock-step ``tiled_sample`` runs
(same-sized batch, mixed-size list, EDM) whose images carry different labels.  Every image must come out bit-identical to a
run of its own with its own ``[1]`` label - the conditioning rows of a label are computed by the launches a one-label run
makes - through split launches, step lanes and replayed step graphs.  Un-tiled ``sample()`` keeps refusing differing labels."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import srgd_oracle as O
from srgd_amd import _lib
from srgd_amd.synth import synth_state_dict
from tests.golden import cases as GC
from tests.test_engine_gpu import _schema, build_sampler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _labels(ids):
    return torch.tensor(list(ids)).cuda()


def _group_and_solo(run, conds, labels, seed=7):
    """``run(condition_x, class_label)`` on the whole group with one label per image, then on every image alone with its own
    ``[1]`` label, each after the same reseed; returns (group outputs, solo outputs) as lists of CPU tensors."""
    def reseed():
        torch.manual_seed(seed)
    reseed()
    out = run(conds, _labels(labels))
    group = [o.cpu() for o in out] if isinstance(out, (list, tuple)) else [o[None].cpu() for o in out]
    solo = []
    for i, lb in enumerate(labels):
        reseed()
        c = conds[i] if isinstance(conds, (list, tuple)) else conds[i:i + 1]
        solo.append(run(c, _labels([lb])).cpu())
    return group, solo


def _assert_same(group, solo, what=""):
    assert len(group) == len(solo)
    for i, (g_, s_) in enumerate(zip(group, solo)):
        assert g_.shape == s_.shape and torch.isfinite(g_).all(), (what, i)
        assert torch.equal(g_, s_), (what, i, float((g_ - s_).abs().max()))


# ---------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("precision", ["fp32", "f16x3", "bf16"])
def test_forward_with_one_label_per_sample_is_the_single_label_rows(precision):
    sampler = build_sampler(16)
    unet = sampler.model
    b, labels = 4, [2, 0, 1, 0]
    x = (_rand((b, 3, 128, 128), 21) * 2 - 1).cuda()
    cond = (_rand((b, 3, 128, 128), 22) * 2 - 1).cuda()
    ls = torch.tensor([-3.0, 2.5, 0.75, -1.0]).cuda()
    unet.precision = precision
    try:
        got = unet(x, ls, _labels(labels), cond).cpu()
        # four single-label calls on the same batch: sample i of the call with label i's [1] tensor
        for i, lb in enumerate(labels):
            one = unet(x, ls, _labels([lb]), cond).cpu()
            assert torch.equal(got[i], one[i]), (i, float((got[i] - one[i]).abs().max()))
        assert not torch.equal(got[0], unet(x, ls, _labels([0]), cond).cpu()[0])      # the label is not ignored
        assert torch.equal(unet(x, ls, _labels([1, 1, 1, 1]), cond).cpu(), unet(x, ls, _labels([1]), cond).cpu())
        with pytest.raises(ValueError):
            unet(x, ls, _labels([0, 1, 2]), cond)
    finally:
        unet.precision = "fp32"


def test_forward_with_one_label_per_sample_matches_the_oracle():
    sampler = build_sampler(16)
    unet = sampler.model
    b, labels = 4, [2, 0, 1, 0]
    x = _rand((b, 3, 128, 128), 21) * 2 - 1
    cond = _rand((b, 3, 128, 128), 22) * 2 - 1
    ls = torch.tensor([-3.0, 2.5, 0.75, -1.0])
    got = unet(x.cuda(), ls.cuda(), _labels(labels), cond.cuda()).cpu()
    sd = O.strip_model_prefix(synth_state_dict(_schema(16), seed=0))
    with torch.inference_mode():
        want = O.unet_forward(sd, O.UnetCfg(dim=16), x, ls, torch.tensor(labels), cond)
    err = (got - want).abs().max().item()
    scale = max(1.0, want.abs().max().item())
    print(f"forward [B] labels, fp32 vs oracle: max|diff| = {err:.3e} (eps range {scale:.3f})")
    # the bound test_engine_gpu.py::test_unet_forward_matches_reference applies to its fp32 fixture
    assert err <= 1e-4 * scale, err


# ---------------------------------------------------------------------------------------------- 2. same-sized lock-step
GUIDANCE = {"none": dict(class_cond_scale=1.0),
            "class_from_step_1": dict(class_cond_scale=2.0, class_guidance_start_steps=1),     # one-pass step 0, two-pass after
            "condition": dict(cond_scale=1.5)}


@pytest.mark.parametrize("guidance", list(GUIDANCE))
@pytest.mark.parametrize("precision", ["fp32", "f16x3", "bf16", "fp8_mixed"])
def test_same_sized_lockstep_with_three_labels_is_bitwise_solo(precision, guidance):
    sampler = build_sampler(16)
    conds = _rand((3, 3, 300, 300), 31).cuda()                   # 768^2 canvases: 9 even / 4 odd tiles per image
    labels = [0, 2, 1]
    solo = None
    for batch_size in (7, 27):                                   # 7 splits an image's tiles across launches, 27 spans all images
        run = lambda c, lb: sampler.tiled_sample(batch_size=batch_size, condition_x=c, class_label=lb, num_sample_steps=4,
                                                 precision=precision, **GUIDANCE[guidance])
        group, solo_now = _group_and_solo(run, conds, labels)
        solo = solo or solo_now
        _assert_same(group, solo, (precision, guidance, batch_size))
        _assert_same(solo_now, solo, "solo runs do not depend on batch_size")
    # the labels matter: image 1 under label 0 is another image
    torch.manual_seed(7)
    other = sampler.tiled_sample(batch_size=27, condition_x=conds[1:2], class_label=_labels([0]), num_sample_steps=4,
                                 precision=precision, **GUIDANCE[guidance]).cpu()
    assert not torch.equal(other, solo[1])


def test_same_sized_lockstep_device_noise_and_q_start():
    sampler = build_sampler(16)
    conds = _rand((3, 3, 300, 300), 32).cuda()
    sampler.noise_source = "device"
    sampler.device_noise_seed = 5
    try:
        run = lambda c, lb: sampler.tiled_sample(batch_size=10, condition_x=c, class_label=lb, num_sample_steps=5,
                                                 generation_start_steps=1, class_cond_scale=1.5, precision="bf16")
        group, solo = _group_and_solo(run, conds, [1, 0, 2])
    finally:
        sampler.noise_source = "host"
    _assert_same(group, solo)


# ---------------------------------------------------------------------------------------------- 3. mixed-size list
@pytest.mark.parametrize("noise,precision,kw", [
    ("host", "fp32", dict(batch_size=7, generation_start_steps=1, num_sample_steps=4)),
    ("device", "bf16", dict(batch_size=100, class_cond_scale=1.3, class_guidance_start_steps=1, num_sample_steps=3)),
    ("device", "f16x3", dict(batch_size=7, cond_scale=1.5, num_sample_steps=3))])
def test_mixed_size_group_with_labels_is_bitwise_solo(noise, precision, kw):
    sampler = build_sampler(16)
    sizes = [(256, 256), (480, 320), (320, 480), (384, 384), (480, 320)]      # the group of test_mixed_lockstep_gpu.py
    labels = [1, 0, 2, 2, 1]                                                  # 480x320 twice (one noise class), labels 0 and 1
    g = torch.Generator().manual_seed(11)
    conds = [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in sizes]
    sampler.noise_source = noise
    sampler.device_noise_seed = 7
    try:
        run = lambda c, lb: sampler.tiled_sample(condition_x=c, class_label=lb, precision=precision, **kw)
        group, solo = _group_and_solo(run, conds, labels)
    finally:
        sampler.noise_source = "host"
    _assert_same(group, solo, (noise, precision))
    for (h, w), o in zip(sizes, group):
        assert o.shape == (1, 3, h, w)


# ---------------------------------------------------------------------------------------------- 4. EDM
def _edm(sampler, steps):
    from srgd_amd.model import ConditionalElucidatedDiffusionSR
    return ConditionalElucidatedDiffusionSR(sampler.model, image_size=256, num_sample_steps=steps).eval()


@pytest.mark.parametrize("precision,kw", [("fp32", dict(batch_size=7)),
                                          ("bf16", dict(batch_size=27, class_cond_scale=2.0, class_guidance_start_steps=1)),
                                          ("f16x3", dict(batch_size=5, cond_scale=1.5))])
def test_edm_heun_lockstep_with_labels_is_bitwise_solo(precision, kw):
    sampler = build_sampler(16)
    edm = _edm(sampler, 4)
    conds = _rand((3, 3, 300, 300), 41).cuda()
    run = lambda c, lb: edm.tiled_sample(condition_x=c, class_label=lb, precision=precision, **kw)
    group, solo = _group_and_solo(run, conds, [2, 0, 1])
    _assert_same(group, solo, precision)
    with pytest.raises(NotImplementedError):                     # its mixed-size list stays refused
        edm.tiled_sample(condition_x=[conds[:1], conds[1:2]], class_label=_labels([0, 1]))


def _dpmpp_engine_run(sampler, edm, conds, labels, precision, steps, passes, kind, scale, sub_batch):
    """DPM-Solver++ steps (srgd_edm_dpmpp_step) over ``len(conds)`` one-tile images begun as ONE lock-step run - the un-tiled
    ``sample()`` keeps its one label, so the step is driven through the engine as ``sample_using_dpmpp`` drives it."""
    from srgd_amd.model import SamplerGeometry
    n = conds.shape[0]
    eng = sampler.model.engine(precision)
    _, scalars, c_noise = edm._dpmpp_tables(steps, True)
    geo = SamplerGeometry(H=256, W=256, Hp=256, Wp=256, left=0, top=0, inner_l=0, inner_t=0, inner_r=256, inner_b=256, tile=256,
                          n_even=1, n_odd=1, n_images=n)
    cond_canvas = torch.empty(n, 3, 256, 256, device="cuda")
    eng.edm_begin(geo, conds, cond_canvas, [(0, 0)], [(0, 0)], scalars, c_noise, labels[0])
    if len(set(labels)) > 1:
        eng.sampler_image_labels(labels)
    img = (_rand((1, 3, 256, 256), 43) * 2 - 1).cuda().repeat(n, 1, 1, 1).contiguous()
    old = torch.zeros_like(img)
    for i in range(steps):
        eng.edm_dpmpp_step(i, img, cond_canvas, None, old, passes, kind, scale, sub_batch)
    out = torch.empty(n, 3, 256, 256, device="cuda")
    eng.sampler_end(img, out)
    return out.cpu()


@pytest.mark.parametrize("precision,passes,kind,scale", [("fp32", 1, 0, 1.0), ("bf16", 2, 1, 2.0), ("f16x3", 2, 2, 1.5)])
def test_edm_dpmpp_step_with_labels_is_bitwise_solo(precision, passes, kind, scale):
    sampler = build_sampler(16)
    edm = _edm(sampler, 4)
    conds = _rand((3, 3, 256, 256), 42).cuda()
    labels = [1, 2, 0]
    for sub_batch in (2, 3):
        group = _dpmpp_engine_run(sampler, edm, conds, labels, precision, 4, passes, kind, scale, sub_batch)
        for i, lb in enumerate(labels):
            solo = _dpmpp_engine_run(sampler, edm, conds[i:i + 1].contiguous(), [lb], precision, 4, passes, kind, scale, 1)
            assert torch.equal(group[i], solo[0]), (sub_batch, i, float((group[i] - solo[0]).abs().max()))
    assert not torch.equal(group[0], _dpmpp_engine_run(sampler, edm, conds[:1].contiguous(), [0], precision, 4, passes, kind,
                                                       scale, 1)[0])


# ---------------------------------------------------------------------------------------------- 5. lanes
def test_step_lanes_carry_the_labels():
    from srgd_amd.lanes import lanes_wanted
    sampler = build_sampler(16)
    conds = _rand((2, 3, 300, 300), 51).cuda()
    assert lanes_wanted(18, 1, 18, 2, "bf16") == 2
    keep = sampler.step_lanes
    sampler.noise_source = "device"
    sampler.device_noise_seed = 3
    outs = {}
    try:
        for lanes in (1, 2):
            sampler.step_lanes = lanes
            run = lambda c, lb: sampler.tiled_sample(batch_size=18, condition_x=c, class_label=lb, num_sample_steps=4,
                                                     class_cond_scale=1.5, precision="bf16")
            outs[lanes] = _group_and_solo(run, conds, [2, 0])
            # the mixed-size form and EDM start their further engines the same way
            listed = _group_and_solo(run, [conds[:1], conds[1:2]], [2, 0])[0]
            _assert_same(listed, outs[lanes][0], ("list form", lanes))
        edm = _edm(sampler, 4)
        edm.noise_source, edm.device_noise_seed, edm.step_lanes = "device", 3, 2
        run = lambda c, lb: edm.tiled_sample(batch_size=18, condition_x=c, class_label=lb, precision="bf16")
        _assert_same(*_group_and_solo(run, conds, [1, 2]), "edm, two lanes")
    finally:
        sampler.step_lanes = keep
        sampler.noise_source = "host"
    _assert_same(*outs[2], "two lanes")
    _assert_same(outs[2][0], outs[1][0], "two lanes against one")


# ---------------------------------------------------------------------------------------------- 6. graph reuse
def test_one_engine_replays_its_step_graphs_under_changing_labels():
    sampler = build_sampler(16)
    conds = _rand((2, 3, 300, 300), 61).cuda()
    keep = sampler.step_lanes
    sampler.noise_source = "device"
    sampler.device_noise_seed = 9
    sampler.step_lanes = 1
    try:
        # 8 steps: each (parity, guidance) key runs eagerly once, is captured on its second occurrence and replayed after
        run = lambda c, lb: sampler.tiled_sample(batch_size=18, condition_x=c, class_label=lb, num_sample_steps=8,
                                                 class_cond_scale=1.5, precision="bf16")
        solo = {(i, lb): run(conds[i:i + 1], _labels([lb])).cpu() for i in (0, 1) for lb in (0, 1)}
        for labels in ([0, 1], [1, 0], [1, 1]):
            out = run(conds, _labels(labels)).cpu()
            for i, lb in enumerate(labels):
                assert torch.equal(out[i:i + 1], solo[i, lb]), (labels, i)
        assert torch.equal(out, run(conds, _labels([1])).cpu())          # [1, 1] is today's [1]-label run
        os.environ["SRGD_GRAPHS"] = "0"                                  # and the replayed steps equal eager ones
        sampler.model._invalidate_engines()
        assert torch.equal(run(conds, _labels([1, 0])).cpu(), torch.cat([solo[0, 1], solo[1, 0]]))
    finally:
        os.environ.pop("SRGD_GRAPHS", None)
        sampler.model._invalidate_engines()
        sampler.step_lanes = keep
        sampler.noise_source = "host"


# ---------------------------------------------------------------------------------------------- 7. unchanged behaviour
def test_equal_labels_and_untiled_sample_behave_as_before():
    sampler = build_sampler(16)
    conds = _rand((2, 3, 300, 300), 71).cuda()
    outs = []
    for lb in ([2], [2, 2]):
        torch.manual_seed(4)
        outs.append(sampler.tiled_sample(batch_size=8, condition_x=conds, class_label=_labels(lb), num_sample_steps=3).cpu())
    assert torch.equal(outs[0], outs[1])
    torch.manual_seed(4)
    listed = sampler.tiled_sample(batch_size=8, condition_x=[conds[:1], conds[1:2]], class_label=_labels([2, 2]), num_sample_steps=3)
    assert torch.equal(torch.cat([o.cpu() for o in listed]), outs[0])
    cond = _rand((2, 3, 256, 256), 72).cuda()
    with pytest.raises(NotImplementedError):
        sampler.sample(batch_size=2, condition_x=cond, class_label=_labels([0, 2]), num_sample_steps=2)
    edm = _edm(sampler, 3)
    with pytest.raises(NotImplementedError):
        edm.sample(batch_size=2, condition_x=cond, class_label=_labels([0, 2]))
    # one canvas sharded over ranks: differing labels are refused, never collapsed to the first
    sampler.canvas_group = object()
    try:
        with pytest.raises(NotImplementedError):
            sampler.tiled_sample(batch_size=8, condition_x=conds, class_label=_labels([0, 2]), num_sample_steps=2)
    finally:
        sampler.canvas_group = None


# ---------------------------------------------------------------------------------------------- 8. errors
def test_label_errors_are_reported_and_leave_the_engine_usable():
    sampler = build_sampler(16)
    conds = _rand((2, 3, 300, 300), 81).cuda()
    kw = dict(batch_size=8, condition_x=conds, num_sample_steps=2)
    torch.manual_seed(1)
    want = sampler.tiled_sample(class_label=_labels([0, 1]), **kw).cpu()
    for bad in ([0, 3], [-1, 1]):
        with pytest.raises(_lib.SrgdHipError, match="out of range"):
            sampler.tiled_sample(class_label=_labels(bad), **kw)
    with pytest.raises(_lib.SrgdHipError, match="out of range"):
        sampler.tiled_sample(batch_size=8, condition_x=[conds[:1], conds[1:2]], class_label=_labels([0, 7]), num_sample_steps=2)
    for count in (3, 4):
        with pytest.raises(ValueError):
            sampler.tiled_sample(class_label=_labels(range(count)), **kw)
    with pytest.raises(ValueError):
        sampler.tiled_sample(batch_size=8, condition_x=[conds[:1], conds[1:2]], class_label=_labels([0, 1, 2]), num_sample_steps=2)
    edm = _edm(sampler, 3)
    with pytest.raises(ValueError):
        edm.tiled_sample(batch_size=8, condition_x=conds, class_label=_labels([0, 1, 2]))
    x, ls = torch.zeros(2, 3, 64, 64).cuda(), torch.zeros(2).cuda()
    with pytest.raises(_lib.SrgdHipError, match="out of range"):
        sampler.model(x, ls, _labels([0, 3]), None)
    # the C ABI: no begun run, wrong image count, a call after the first step
    eng = sampler.model.engine("fp32")
    sampler.tiled_sample(class_label=_labels([0]), **kw)             # leaves an ended run behind; labels need a begun one
    with pytest.raises(_lib.SrgdHipError, match="srgd_sampler_begin"):
        eng.sampler_image_labels([0, 1])
    from srgd_amd.model import SamplerGeometry, _schedule
    scalars, log_snrs = _schedule(2)
    geo = SamplerGeometry(H=256, W=256, Hp=256, Wp=256, left=0, top=0, inner_l=0, inner_t=0, inner_r=256, inner_b=256, tile=256,
                          n_even=1, n_odd=1, n_images=2)
    cond01, canvas = _rand((2, 3, 256, 256), 82).cuda(), torch.empty(2, 3, 256, 256, device="cuda")
    eng.sampler_begin(geo, cond01, canvas, [(0, 0)], [(0, 0)], scalars, log_snrs, 0)
    with pytest.raises(_lib.SrgdHipError, match="one label per image"):
        eng.sampler_image_labels([0, 1, 2])
    eng.sampler_image_labels([0, 1])
    eng.sampler_image_labels([2, 1])                                 # before the first step the labels may still change
    img = torch.zeros(2, 3, 256, 256, device="cuda")
    eng.sampler_step(0, img, canvas, None, None, None, 1, 0, 1.0, 2, seed=1)
    with pytest.raises(_lib.SrgdHipError, match="taken a step"):
        eng.sampler_image_labels([0, 1])
    eng.sampler_end(img, torch.empty(2, 3, 256, 256, device="cuda"))
    torch.cuda.synchronize()
    # after all of that a normal run gives what it gave
    torch.manual_seed(1)
    assert torch.equal(sampler.tiled_sample(class_label=_labels([0, 1]), **kw).cpu(), want)


def test_labels_on_a_unet_without_class_embedding_raise():
    from srgd_amd.model import ConditionalContinuousTimeGaussianDiffusionSR, ConditionalSRUnet
    torch.manual_seed(0)
    unet = ConditionalSRUnet(16, learned_sinusoidal_cond=True, learned_sinusoidal_dim=32, num_classes=None).eval().cuda()
    sampler = ConditionalContinuousTimeGaussianDiffusionSR(unet, image_size=256, num_sample_steps=2).eval()
    conds = _rand((2, 3, 256, 256), 91).cuda()
    x, ls = torch.zeros(2, 3, 64, 64).cuda(), torch.zeros(2).cuda()
    with pytest.raises(_lib.SrgdHipError, match="no class embedding"):
        unet(x, ls, _labels([0, 1]), None)
    with pytest.raises(_lib.SrgdHipError, match="no class embedding"):
        sampler.tiled_sample(batch_size=2, condition_x=conds, class_label=_labels([0, 1]), num_sample_steps=2)
    out = sampler.tiled_sample(batch_size=2, condition_x=conds, class_label=None, num_sample_steps=2)   # and it still runs
    assert torch.isfinite(out).all() and tuple(out.shape) == (2, 3, 256, 256)


# ---------------------------------------------------------------------------------------------- 9. CLI
def test_cli_label_file_writes_the_pngs_of_single_image_runs(tmp_path):
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    rng = np.random.default_rng(8)
    files = {"a.png": ((120, 80), 0), "b.png": ((80, 120), 2), "c.png": ((64, 64), 1)}     # LR (w, h), label
    indir = tmp_path / "in"
    indir.mkdir()
    for name, ((w, h), _) in files.items():
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(indir / name)
    label_file = tmp_path / "labels.txt"
    label_file.write_text("a.png 0\nb.png 2\n")                      # c.png takes --test_label

    def cli(input_dir, outdir, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(input_dir),
               "--output_dir", str(outdir), "--num_sample_steps", "3", "--seed", "71", "--batch_size", "4", *extra]
        return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    r = cli(indir, tmp_path / "group", "--test_label", "1", "--label_file", str(label_file), "--lockstep_tiles", "64")
    assert r.returncode == 0, r.stderr[-3000:]
    assert "lock-step group: 3 images" in r.stdout, r.stdout[-2000:]
    for name, (_, label) in files.items():
        one = tmp_path / f"in_{name}"
        one.mkdir()
        (one / name).write_bytes((indir / name).read_bytes())
        r1 = cli(one, tmp_path / f"solo_{name}", "--test_label", str(label))
        assert r1.returncode == 0, r1.stderr[-3000:]
        out = name.replace(".png", "_out.png")
        assert (tmp_path / "group" / out).read_bytes() == (tmp_path / f"solo_{name}" / out).read_bytes(), name
    # a label outside the model's classes ends the run before any GPU work
    label_file.write_text("a.png 3\n")
    r = cli(indir, tmp_path / "bad", "--label_file", str(label_file))
    assert r.returncode != 0 and "outside [0, 3)" in r.stderr and not (tmp_path / "bad").exists()
