"""Per-image noise seeds in lock-step on the GPU: ``tiled_sample(seeds=...)`` gives every image of a group the noise of a solo
run with its own seed - bit-identical outputs for host and device noise, every precision, guidance, q_sample starts, per-image
labels, step lanes and hipGraph replay - and the batched Philox kernel behind it (srgd_randn_streams) writes, stream by stream,
exactly what the single-stream kernel (srgd_randn) writes.  Every comparison is ``torch.equal``."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import _lib
from srgd_amd.synth import synth_state_dict
from tests.test_engine_gpu import _schema, build_sampler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 256^2 (1 tile), 480x320 twice and 320x480 (768^2 canvases): seeds 5, 5, 9, 5 -> streams (256^2, 5), (768^2, 5), (768^2, 9)
SIZES = [(256, 256), (480, 320), (480, 320), (320, 480)]
SEEDS = [5, 5, 9, 5]


def _conds(sizes, seed=11):
    g = torch.Generator().manual_seed(seed)
    conds = [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in sizes]
    for i, s in enumerate(sizes):                               # a repeated size is the SAME image (K samples of one image)
        j = list(sizes).index(s)
        conds[i] = conds[j]
    return conds


def _solo(sampler, cond, seed, **kw):
    """The contract's solo call: that image alone after torch.manual_seed(seed) / with device_noise_seed = seed."""
    torch.manual_seed(seed)
    sampler.device_noise_seed = seed
    return sampler.tiled_sample(condition_x=cond, **kw).cpu()


def _seeded_and_solo(sampler, conds, seeds, labels=None, **kw):
    torch.manual_seed(12345)                                    # neither the caller's generator nor device_noise_seed may matter
    sampler.device_noise_seed = 999
    before = torch.get_rng_state()
    group_label = None if labels is None else torch.tensor(labels).cuda()
    group = [o.cpu() for o in sampler.tiled_sample(condition_x=conds, seeds=seeds, class_label=group_label, **kw)]
    if sampler.noise_source == "host":
        assert torch.equal(torch.get_rng_state(), before), "a seeded run must not read or advance the caller's generator"
    solo = [_solo(sampler, c, s, class_label=None if labels is None else torch.tensor([labels[i % len(labels)]]).cuda(), **kw)
            for i, (c, s) in enumerate(zip(conds, seeds))]           # labels: one for all images or one per image
    return group, solo


# ------------------------------------------------------------------------------------------- 1. the batched kernel
def test_batched_philox_equals_the_single_stream_kernel():
    eng = build_sampler(16).model.engine("fp32")
    counts = [1, 5, 1023, 3 * 256 * 256, 3 * 768 * 768]
    seeds = [71, 2 ** 63 + 5, 0, 123456789012345, 9]
    stream_id = (1 << 32) | 0x80000000
    offsets, off = [], 0
    for n in counts:                                            # back to back with one guard element after every slice
        offsets.append(off)
        off += n + 1
    assert any(o % 4 for o in offsets)
    guard = -12345.0
    dst = torch.full((off,), guard, device="cuda")
    eng.randn_streams_(dst, offsets, counts, seeds, stream_id)
    torch.cuda.synchronize()
    for o, n, s in zip(offsets, counts, seeds):
        want = eng.randn_(torch.empty(n, device="cuda"), s, stream_id)
        assert torch.equal(dst[o:o + n], want), (n, s)
        assert float(dst[o + n]) == guard, (n, "guard overwritten")
    assert torch.isfinite(dst).all()
    assert not torch.equal(dst[offsets[3]:offsets[3] + 1023], dst[offsets[2]:offsets[2] + 1023])     # distinct seeds, distinct noise
    # a single-stream call, at an odd offset
    one = torch.full((1 + 1023 + 1,), guard, device="cuda")
    eng.randn_streams_(one, [1], [1023], [42], 3)
    assert torch.equal(one[1:1024], eng.randn_(torch.empty(1023, device="cuda"), 42, 3))
    assert float(one[0]) == guard and float(one[-1]) == guard
    # misuse is an error, not a launch
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.srgd_randn_streams(C.c_void_p(one.data_ptr()), None, None, None, 1, 0, st) != 0
    assert L.srgd_randn_streams(C.c_void_p(one.data_ptr()), (C.c_int64 * 1)(-4), (C.c_int64 * 1)(4), (C.c_uint64 * 1)(1), 1, 0, st) != 0
    assert b"srgd_randn_streams" in L.srgd_last_error()


# ------------------------------------------------------------------------------------------- 2. group == solo runs
@pytest.mark.parametrize("noise,precision,batch_size,class_scale", [("host", "fp32", 7, 1.0), ("device", "bf16", 100, 1.3),
                                                                     ("device", "f16x3", 7, 1.0)])
def test_seeded_group_is_bitwise_its_solo_runs(noise, precision, batch_size, class_scale):
    sampler = build_sampler(16)
    conds = _conds(SIZES)
    sampler.noise_source = noise
    try:
        group, solo = _seeded_and_solo(sampler, conds, SEEDS, labels=[1], batch_size=batch_size, num_sample_steps=3,
                                       class_cond_scale=class_scale, precision=precision)
    finally:
        sampler.noise_source = "host"
    for i, (m, s) in enumerate(zip(group, solo)):
        assert m.shape == (1, 3) + SIZES[i] and torch.isfinite(m).all()
        assert torch.equal(m, s), (i, SIZES[i], SEEDS[i], float((m - s).abs().max()))
    assert not torch.equal(group[1], group[2])                  # the same image with seeds 5 and 9: two samples


# ------------------------------------------------------------------------------------------- 3. the [B,3,H,W] form
@pytest.mark.parametrize("noise", ["host", "device"])
def test_seeded_batch_tensor_form(noise):
    sampler = build_sampler(16)
    one = torch.rand(1, 3, 300, 300, generator=torch.Generator().manual_seed(2)).cuda()
    kw = dict(batch_size=9, class_label=torch.tensor([0]).cuda(), num_sample_steps=3, precision="fp32")
    sampler.noise_source = noise
    try:
        out = sampler.tiled_sample(condition_x=one.repeat(3, 1, 1, 1), seeds=[1, 2, 1], **kw)
        assert torch.is_tensor(out) and out.shape == (3, 3, 300, 300)
        out = out.cpu()
        solos = [_solo(sampler, one, s, **kw) for s in (1, 2)]
    finally:
        sampler.noise_source = "host"
    assert torch.equal(out[0], out[2]) and not torch.equal(out[0], out[1])
    assert torch.equal(out[0:1], solos[0]) and torch.equal(out[1:2], solos[1])


# ------------------------------------------------------------------------------------------- 4. no drift from today
@pytest.mark.parametrize("noise,precision", [("host", "fp32"), ("device", "bf16")])
def test_equal_seeds_reproduce_the_unseeded_group(noise, precision):
    sampler = build_sampler(16)
    conds = _conds(SIZES)
    kw = dict(batch_size=11, class_label=torch.tensor([2]).cuda(), num_sample_steps=3, precision=precision)
    s = 31
    sampler.noise_source = noise
    try:
        torch.manual_seed(s)
        sampler.device_noise_seed = s
        unseeded = [o.cpu() for o in sampler.tiled_sample(condition_x=conds, **kw)]
        torch.manual_seed(0)
        sampler.device_noise_seed = 0
        seeded = [o.cpu() for o in sampler.tiled_sample(condition_x=conds, seeds=[s] * len(conds), **kw)]
    finally:
        sampler.noise_source = "host"
    assert all(torch.equal(a, b) for a, b in zip(seeded, unseeded))


# ------------------------------------------------------------------------------------------- 5. q_sample starts
def test_seeded_q_start_and_late_guidance_are_bitwise_solo():
    sampler = build_sampler(16)
    sizes, seeds = [(480, 320), (256, 256), (480, 320)], [3, 3, 8]
    conds = _conds(sizes, seed=5)
    group, solo = _seeded_and_solo(sampler, conds, seeds, labels=[0], batch_size=6, num_sample_steps=5, generation_start_steps=1,
                                   cond_scale=1.5, guidance_start_steps=3, precision="fp32")
    assert all(torch.equal(m, s) for m, s in zip(group, solo))
    assert not torch.equal(group[0], group[2])
    sampler.noise_source = "device"
    try:
        group, solo = _seeded_and_solo(sampler, conds, seeds, labels=[0], batch_size=6, num_sample_steps=3,
                                       start_white_noise=False, precision="bf16")
    finally:
        sampler.noise_source = "host"
    assert all(torch.equal(m, s) for m, s in zip(group, solo))
    assert not torch.equal(group[0], group[2])


# ------------------------------------------------------------------------------------------- 6. lanes and graphs
def test_seeded_group_lanes_and_graphs_do_not_change_it():
    sampler = build_sampler(16)
    sizes, seeds = [(320, 480), (256, 256), (320, 480)], [4, 4, 6]
    conds = _conds(sizes, seed=9)
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
                outs[graphs, lanes] = [o.cpu() for o in sampler.tiled_sample(
                    batch_size=19, condition_x=conds, class_label=label, num_sample_steps=4, precision="bf16", seeds=seeds)]
    finally:
        os.environ.pop("SRGD_GRAPHS", None)
        sampler.model._invalidate_engines()
        sampler.step_lanes = keep
        sampler.noise_source = "host"
    ref = outs["1", 1]
    for key, got in outs.items():
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), key
    assert not torch.equal(ref[0], ref[2])


# ------------------------------------------------------------------------------------------- 7. seeds + per-image labels
@pytest.mark.parametrize("noise,precision,class_scale", [("host", "fp32", 1.0), ("device", "bf16", 1.3)])
def test_seeds_together_with_per_image_labels(noise, precision, class_scale):
    sampler = build_sampler(16)
    sizes, seeds, labels = [(256, 256), (480, 320), (480, 320), (256, 256)], [7, 7, 2, 7], [0, 2, 2, 1]
    conds = _conds(sizes, seed=13)
    sampler.noise_source = noise
    try:
        group, solo = _seeded_and_solo(sampler, conds, seeds, labels=labels, batch_size=8, num_sample_steps=3,
                                       class_cond_scale=class_scale, precision=precision)
    finally:
        sampler.noise_source = "host"
    for i, (m, s) in enumerate(zip(group, solo)):
        assert torch.equal(m, s), (i, labels[i], seeds[i])
    assert not torch.equal(group[0], group[3])                  # same image, same seed, different labels
    assert not torch.equal(group[1], group[2])                  # same image, same label, different seeds


# ------------------------------------------------------------------------------------------- 8. Python refusals
def test_python_refusals():
    sampler = build_sampler(16)
    conds = _conds([(256, 256), (480, 320)])
    batch = torch.rand(2, 3, 256, 256).cuda()
    kw = dict(num_sample_steps=2)
    for cond in (conds, batch):
        with pytest.raises(ValueError, match="one per image"):
            sampler.tiled_sample(condition_x=cond, seeds=[1, 2, 3], **kw)
        with pytest.raises(ValueError, match="outside"):
            sampler.tiled_sample(condition_x=cond, seeds=[1, -2], **kw)
        with pytest.raises(ValueError, match="not an integer"):
            sampler.tiled_sample(condition_x=cond, seeds=[1, 2.5], **kw)
        with pytest.raises(NotImplementedError, match="with_images"):
            sampler.tiled_sample(condition_x=cond, seeds=[1, 2], with_images=True, **kw)
        with pytest.raises(NotImplementedError, match="with_images"):
            sampler.tiled_sample(condition_x=cond, seeds=[1, 2], with_x0_images=True, **kw)
        sampler.canvas_group = object()
        try:
            with pytest.raises(NotImplementedError, match="canvas_group"):
                sampler.tiled_sample(condition_x=cond, seeds=[1, 2], **kw)
        finally:
            sampler.canvas_group = None
    from srgd_amd.model import ConditionalElucidatedDiffusionSR
    edm = ConditionalElucidatedDiffusionSR(sampler.model, image_size=256, num_sample_steps=2)
    with pytest.raises(NotImplementedError, match="seeds"):
        edm.tiled_sample(condition_x=batch, seeds=[1, 2])
    with pytest.raises(NotImplementedError):                    # the list form stays refused there, seeds or not
        edm.tiled_sample(condition_x=conds, seeds=[1, 2])
    assert "seeds" not in __import__("inspect").signature(sampler.sample).parameters       # un-tiled sample(): per-image noise already


# ------------------------------------------------------------------------------------------- 9. C-ABI refusals
def test_cabi_refusals_leave_the_engine_usable():
    from srgd_amd.model import ConditionalElucidatedDiffusionSR, _schedule
    L = _lib.lib()
    sampler = build_sampler(16)
    cfg = _lib.UnetConfig()
    cfg.dim, cfg.n_stages, cfg.channels, cfg.groups, cfg.heads, cfg.dim_head = 16, 4, 3, 8, 4, 32
    cfg.sinus_dim, cfg.num_classes, cfg.precision, cfg.device = 32, 3, 0, 0
    for i, (m, f) in enumerate(zip((1, 2, 4, 8), (0, 0, 0, 1))):
        cfg.dim_mults[i], cfg.full_attn[i] = m, f
    h = C.c_void_p()
    assert L.srgd_create(C.byref(cfg), C.byref(h)) == 0
    for k, v in synth_state_dict(_schema(16), seed=0).items():
        t = v.float().contiguous()
        shp = (C.c_int64 * max(1, t.dim()))(*t.shape)
        assert L.srgd_load_weight(h, k.encode(), C.c_void_p(t.data_ptr()), shp, t.dim()) == 0, L.srgd_last_error()
    assert L.srgd_finalize_weights(h) == 0, L.srgd_last_error()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def err(rc):
        assert rc != 0
        msg = L.srgd_last_error().decode()
        assert "srgd_sampler_noise_seeds" in msg
        return msg

    one, two = (C.c_uint64 * 1)(3), (C.c_uint64 * 2)(3, 4)
    assert "begin" in err(L.srgd_sampler_noise_seeds(h, one, 1, st))                       # before any begin
    geo = _lib.SamplerGeometry(H=256, W=256, Hp=256, Wp=256, left=0, top=0, inner_l=0, inner_t=0, inner_r=256, inner_b=256,
                               tile=256, n_even=1, n_odd=1, n_images=2)
    tile0 = (C.c_int32 * 2)(0, 0)
    scalars, log_snrs = _schedule(2)
    sc, lsn = (_lib.StepScalars * 2)(*scalars), (C.c_float * 2)(*log_snrs)
    cond = torch.rand(2, 3, 256, 256, device="cuda")
    cc, img = torch.zeros(2, 3, 256, 256, device="cuda"), torch.randn(2, 3, 256, 256, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                                 # noqa: E731
    begin = lambda: L.srgd_sampler_begin(h, C.byref(geo), p(cond), p(cc), tile0, tile0, 2, sc, lsn, 0, st)   # noqa: E731
    assert begin() == 0, L.srgd_last_error()
    assert "one seed per noise class" in err(L.srgd_sampler_noise_seeds(h, two, 2, st))    # a same-sized run has one class
    assert "null" in err(L.srgd_sampler_noise_seeds(h, None, 1, st))
    assert L.srgd_sampler_step(h, 0, p(img), p(cc), None, None, None, 1, 0, 1.0, 4, 1, st) == 0, L.srgd_last_error()
    assert "step" in err(L.srgd_sampler_noise_seeds(h, one, 1, st))                        # after a step
    # an EDM run
    edm = ConditionalElucidatedDiffusionSR(sampler.model, image_size=256, num_sample_steps=2)
    _, _, esc, c_noise = edm._step_tables(2, True)
    esc_c, cn = (_lib.EdmScalars * 2)(*esc), (C.c_float * 4)(*[float(v) for v in c_noise])
    assert L.srgd_edm_begin(h, C.byref(geo), p(cond), p(cc), tile0, tile0, 2, esc_c, cn, 0, st) == 0, L.srgd_last_error()
    assert "EDM" in err(L.srgd_sampler_noise_seeds(h, one, 1, st))
    # ... and the engine still works: a seeded run of two images that share the stream equals the same run seeded per step
    outs = []
    for seeded in (True, False):
        assert begin() == 0, L.srgd_last_error()
        if seeded:
            assert L.srgd_sampler_noise_seeds(h, one, 1, st) == 0, L.srgd_last_error()
        x = img.clone()
        for step in range(2):
            assert L.srgd_sampler_step(h, step, p(x), p(cc), None, None, None, 1, 0, 1.0, 4, 77 if seeded else 3, st) == 0, \
                L.srgd_last_error()
        out = torch.empty(2, 3, 256, 256, device="cuda")
        assert L.srgd_sampler_end(h, p(x), p(out), st) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])         # seeds {3} with the step's seed 77 ignored == the unseeded run with seed 3
    assert L.srgd_destroy(h) == 0


# ------------------------------------------------------------------------------------------- 10. the command line
def test_cli_samples_writes_the_solo_pngs_of_each_seed(tmp_path):
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    indir = tmp_path / "in"
    indir.mkdir()
    rng = np.random.default_rng(4)
    for name, (h, w) in (("a", (40, 56)), ("b", (64, 48))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(indir / f"{name}.png")

    def run(tag, *extra):
        outdir = tmp_path / tag
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(indir),
               "--output_dir", str(outdir), "--num_sample_steps", "2", "--test_label", "1", "--batch_size", "4", "--device_noise",
               *extra]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)       # one child at a time
        assert r.returncode == 0, r.stderr[-3000:]
        return {f: np.asarray(Image.open(outdir / f).convert("RGB")) for f in sorted(os.listdir(outdir))}

    both = run("samples", "--seed", "71", "--samples", "2")
    assert sorted(both) == ["a_out.png", "a_out_s1.png", "b_out.png", "b_out_s1.png"]
    seed0 = run("seed71", "--seed", "71")
    seed1 = run("seed72", "--seed", "72")
    for n in "ab":
        assert np.array_equal(both[f"{n}_out.png"], seed0[f"{n}_out.png"]), n
        assert np.array_equal(both[f"{n}_out_s1.png"], seed1[f"{n}_out.png"]), n
        assert not np.array_equal(both[f"{n}_out.png"], both[f"{n}_out_s1.png"]), n
