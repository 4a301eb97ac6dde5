"""Mixed-size lock-step on the GPU: images of different sizes sampled together (tiled_sample with a list condition,
srgd_sampler_begin_images) come out bit-identical to their solo runs - host and device noise, guidance, q_sample starts, step
lanes, hipGraph replay - and the 256^2 member of a group matches the reference's own fixture."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd.synth import synth_state_dict
from tests.golden import cases as GC
from tests.test_engine_gpu import G, _schema, build_sampler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 256^2 (1 tile), 480x320 and 320x480 (both 768^2 canvases, 9 / 4 tiles), 384^2 (768^2 too), a repeated 480x320
SIZES = [(256, 256), (480, 320), (320, 480), (384, 384), (480, 320)]


def _conds(sizes, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in sizes]


def _mixed_and_solo(sampler, conds, seed=7, **kw):
    """The group in one call, then every image alone with the same seed; returns (group outputs, solo outputs) on the CPU."""
    torch.manual_seed(seed)
    sampler.device_noise_seed = seed
    mixed = [o.cpu() for o in sampler.tiled_sample(condition_x=conds, **kw)]
    after_group = torch.get_rng_state()
    solo = []
    for i, c in enumerate(conds):
        torch.manual_seed(seed)
        solo.append(sampler.tiled_sample(condition_x=c, **kw).cpu())
        if i == 0 and sampler.noise_source == "host":          # documented: the group leaves the first image's end state
            assert torch.equal(torch.get_rng_state(), after_group)
    return mixed, solo


@pytest.mark.parametrize("noise,precision,batch_size,class_scale", [("host", "fp32", 7, 1.0), ("device", "bf16", 100, 1.3),
                                                                     ("device", "f16x3", 7, 1.0)])
def test_mixed_group_is_bitwise_its_solo_runs(noise, precision, batch_size, class_scale):
    sampler = build_sampler(16)
    conds = _conds(SIZES)
    label = torch.tensor([1]).cuda()
    sampler.noise_source = noise
    try:
        mixed, solo = _mixed_and_solo(sampler, conds, batch_size=batch_size, class_label=label, num_sample_steps=3,
                                      class_cond_scale=class_scale, precision=precision)
    finally:
        sampler.noise_source = "host"
    for i, (m, s) in enumerate(zip(mixed, solo)):
        assert m.shape == (1, 3) + SIZES[i] and torch.isfinite(m).all()
        assert torch.equal(m, s), (i, SIZES[i], float((m - s).abs().max()))
    assert not torch.equal(mixed[1], mixed[2].transpose(2, 3))   # different images, not one broadcast


def test_mixed_group_member_matches_the_reference_fixture():
    case = next(c for c in GC.SAMPLER_CASES if c["name"] == "dim16_256_cfg1")
    z = np.load(os.path.join(G, f"sample_{case['name']}.npz"))
    sampler = build_sampler(case["dim"], weight_seed=case["weight_seed"])
    cond = GC.sampler_condition(case).cuda()
    group = _conds([(480, 320)], seed=3) + [cond] + _conds([(320, 480)], seed=4)
    torch.manual_seed(case["seed"])
    sampler.noise_source = "host"
    outs = sampler.tiled_sample(batch_size=case["batch_size"], condition_x=group, class_label=torch.tensor([case["label"]]).cuda(),
                                cond_scale=case["cond_scale"], class_cond_scale=case["class_cond_scale"],
                                num_sample_steps=case["steps"], precision="fp32")
    err = (outs[1].cpu() - torch.from_numpy(z["image"])).abs().max().item()
    assert err <= 1e-3, err
    assert err <= 2e-4, err


def test_mixed_q_start_and_late_guidance_are_bitwise_solo():
    sampler = build_sampler(16)
    conds = _conds([(480, 320), (256, 256), (320, 480)], seed=5)
    label = torch.tensor([0]).cuda()
    mixed, solo = _mixed_and_solo(sampler, conds, batch_size=6, class_label=label, num_sample_steps=5, generation_start_steps=1,
                                  cond_scale=1.5, guidance_start_steps=3, precision="fp32")
    for m, s in zip(mixed, solo):
        assert torch.equal(m, s)
    sampler.noise_source = "device"
    try:
        mixed, solo = _mixed_and_solo(sampler, conds, batch_size=6, class_label=label, num_sample_steps=3,
                                      start_white_noise=False, precision="bf16")
    finally:
        sampler.noise_source = "host"
    for m, s in zip(mixed, solo):
        assert torch.equal(m, s)


def test_mixed_group_lanes_and_graphs_do_not_change_it():
    sampler = build_sampler(16)
    conds = _conds([(320, 480), (256, 256), (384, 384)], seed=9)
    label = torch.tensor([2]).cuda()
    keep = sampler.step_lanes
    outs = {}
    sampler.noise_source = "device"
    try:
        for graphs in ("1", "0"):
            os.environ["SRGD_GRAPHS"] = graphs
            sampler.model._invalidate_engines()                  # the switch is read at engine creation
            for lanes in (1, 2):
                sampler.step_lanes = lanes
                sampler.device_noise_seed = 4
                outs[graphs, lanes] = [o.cpu() for o in sampler.tiled_sample(
                    batch_size=19, condition_x=conds, class_label=label, num_sample_steps=4, precision="bf16")]
    finally:
        os.environ.pop("SRGD_GRAPHS", None)
        sampler.model._invalidate_engines()
        sampler.step_lanes = keep
        sampler.noise_source = "host"
    ref = outs["1", 1]
    for key, got in outs.items():
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), key


def test_mixed_group_dim128_f16x3_device_noise():
    sampler = build_sampler(128)
    conds = [GC.synthetic_lr_condition(0, 64, 64).cuda(), GC.synthetic_lr_condition(1, 80, 120).cuda()]   # 256^2 and 320x480
    sampler.noise_source = "device"
    try:
        mixed, solo = _mixed_and_solo(sampler, conds, batch_size=10, class_label=torch.tensor([0]).cuda(), num_sample_steps=2,
                                      precision="f16x3")
    finally:
        sampler.noise_source = "host"
    for m, s in zip(mixed, solo):
        assert torch.equal(m, s)


def test_mixed_refusals_and_sharding_entries():
    from srgd_amd import _lib
    sampler = build_sampler(16)
    conds = _conds([(256, 256), (480, 320)])
    with pytest.raises(NotImplementedError):
        sampler.tiled_sample(condition_x=conds, num_sample_steps=2, with_images=True)
    with pytest.raises(NotImplementedError):
        sampler.tiled_sample(condition_x=conds, num_sample_steps=2, with_x0_images=True)
    sampler.canvas_group = object()
    try:
        with pytest.raises(NotImplementedError):
            sampler.tiled_sample(condition_x=conds, num_sample_steps=2)
    finally:
        sampler.canvas_group = None
    from srgd_amd.model import ConditionalElucidatedDiffusionSR
    edm = ConditionalElucidatedDiffusionSR(sampler.model, image_size=256, num_sample_steps=2)
    with pytest.raises(NotImplementedError):
        edm.tiled_sample(condition_x=conds)
    # the canvas-sharding entries refuse a mixed run
    from srgd_amd.lockstep import plan_mixed_group
    plans, _ = plan_mixed_group([(256, 256), (480, 320)])
    images = [_lib.SamplerImage(H=p.H, W=p.W, Hp=p.Hp, Wp=p.Wp, left=p.box[0], top=p.box[1], inner_l=p.inner[0], inner_t=p.inner[1],
                                inner_r=p.inner[2], inner_b=p.inner[3], n_even=len(p.coords0), n_odd=len(p.coords1),
                                noise_class=p.noise_class) for p in plans]
    from srgd_amd.model import _schedule
    scalars, ls = _schedule(2)
    eng = sampler.model.engine("fp32")
    cond01 = torch.cat([c.reshape(-1) for c in conds])
    canvas = torch.empty(sum(3 * p.Hp * p.Wp for p in plans), device="cuda")
    eng.sampler_begin_images(256, images, cond01, canvas, [(a, c) for p in plans for (a, _, c, _) in p.coords0],
                             [(a, c) for p in plans for (a, _, c, _) in p.coords1], scalars, ls, -1)
    tiles = torch.empty(1, 3, 256, 256, device="cuda")
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.srgd_sampler_exchange_tiles(eng._h, 0, 0, 1, C.c_void_p(canvas.data_ptr()), C.c_void_p(tiles.data_ptr()), 0, st) != 0
    assert b"srgd_sampler_begin_images" in L.srgd_last_error()
    assert L.srgd_sampler_unpack_gathered(eng._h, 0, 1, 1, 0, 1, C.c_void_p(canvas.data_ptr()), C.c_void_p(tiles.data_ptr()), st) != 0
    out = torch.empty(sum(3 * p.H * p.W for p in plans), device="cuda")
    eng.sampler_end(canvas, out)                                # the run still ends cleanly
    torch.cuda.synchronize()


def test_cli_lockstep_tiles_writes_the_solo_pngs(tmp_path):
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    indir = tmp_path / "in"
    indir.mkdir()
    rng = np.random.default_rng(6)
    for k, (w, h) in enumerate([(120, 80), (80, 120), (64, 64), (120, 80), (96, 96), (80, 120)]):   # LR sizes, x4 below
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(indir / f"img{k}.png")
    outs = {}
    for tag, extra in (("solo", []), ("mixed", ["--lockstep_tiles", "64"])):
        outdir = tmp_path / tag
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(indir),
               "--output_dir", str(outdir), "--num_sample_steps", "3", "--test_label", "1", "--seed", "71", "--batch_size", "4",
               *extra]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[tag] = (r.stdout, {f: (outdir / f).read_bytes() for f in sorted(os.listdir(outdir))})
    assert len(outs["solo"][1]) == 6 and outs["solo"][1] == outs["mixed"][1]
    groups = [ln for ln in outs["mixed"][0].splitlines() if ln.startswith("lock-step group:")]
    assert groups and int(groups[0].split()[2]) > 1, outs["mixed"][0][-2000:]
