"""Per-image noise seeds, host side (no GPU): noise streams of a seeded group (canvas size, seed), the private-generator stream
host noise draws from, the ``--samples`` flag (parsing, output names, grouping, skip-if-exists per sample) and the new C-ABI
declarations."""
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import inference as INF
from srgd_amd.lockstep import image_plan, plan_mixed_group

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")


def test_plan_without_seeds_is_unchanged():
    sizes = [(256, 256), (480, 320), (320, 480)]
    got = plan_mixed_group(sizes)
    assert isinstance(got, tuple) and len(got) == 2
    plans, classes = got
    assert classes == [(256, 256), (768, 768)]
    assert plans == [image_plan(256, 256, 256, 0), image_plan(480, 320, 256, 1), image_plan(320, 480, 256, 1)]
    assert plan_mixed_group(sizes, 256, seeds=None) == got


def test_plan_with_seeds_numbers_noise_streams_by_canvas_and_seed():
    sizes = [(256, 256), (480, 320), (480, 320), (320, 480)]
    plans, classes, class_seeds = plan_mixed_group(sizes, seeds=[5, 5, 9, 5])
    assert [p.noise_class for p in plans] == [0, 1, 2, 1]       # 480x320 and 320x480 share the 768^2 canvas: seed 5 -> one stream
    assert class_seeds == [5, 5, 9]
    assert classes == [(256, 256), (768, 768), (768, 768)]      # canvas of each stream (sizes may repeat)
    unseeded, _ = plan_mixed_group(sizes)
    assert [p._replace(noise_class=0) for p in plans] == [p._replace(noise_class=0) for p in unseeded]   # geometry untouched
    with pytest.raises(ValueError, match="one per image"):
        plan_mixed_group(sizes, seeds=[1, 2])


@pytest.mark.parametrize("seed", [0, 71, 2 ** 40 + 3])
def test_private_generator_reproduces_the_global_seeded_stream(seed):
    state = torch.get_rng_state()
    try:
        torch.manual_seed(seed)
        want = [torch.randn(1, 3, 40, 24), torch.randn(3, 3, 16, 16)]
    finally:
        torch.set_rng_state(state)
    g = torch.Generator().manual_seed(seed)
    got = [torch.randn(1, 3, 40, 24, generator=g), torch.randn(3, 3, 16, 16, generator=g)]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(torch.get_rng_state(), state)            # the private draws left the global generator alone


def _argv(*extra):
    return ["-c", CONF, "-m", "ckpt.pth", "--input_dir", "in", "--output_dir", "out", *extra]


def test_samples_flag_parsing():
    assert INF.parse_args(_argv()).samples == 1
    assert INF.parse_args(_argv("--samples", "3")).samples == 3
    assert INF.parse_args(_argv("--samples", "2", "--lockstep_tiles", "64")).lockstep_tiles == 64
    for bad in ("0", "-2"):
        with pytest.raises(SystemExit, match="--samples"):
            INF.parse_args(_argv("--samples", bad))


def test_sample_output_names():
    assert INF.sample_output_name("/data/in/a.png", 0) == "a_out.png"          # the name a run without --samples writes
    assert INF.sample_output_name("/data/in/a.png", 1) == "a_out_s1.png"
    assert INF.sample_output_name("a.png", 12) == "a_out_s12.png"


def _fake_samplers(monkeypatch, calls):
    def fake(kind):
        def run(images, *a, **kw):
            seeds = a[0] if kind == "seeded" else None
            ims = images if isinstance(images, list) else [images]
            calls.append((kind, [im.size for im in ims], list(seeds) if seeds is not None else kw.get("seed")))
            outs = [Image.new("RGB", (4, 4)) for _ in ims]
            return outs if isinstance(images, list) else outs[0]
        return run
    monkeypatch.setattr(INF, "sr_target_image", fake("solo"))
    monkeypatch.setattr(INF, "sr_target_images", fake("same"))
    monkeypatch.setattr(INF, "sr_target_images_mixed", fake("mixed"))
    monkeypatch.setattr(INF, "sr_target_images_seeded", fake("seeded"))


def _inputs(tmp_path, sizes):
    indir = tmp_path / "in"
    indir.mkdir()
    rng = np.random.default_rng(0)
    for name, (w, h) in sizes.items():
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(indir / f"{name}.png")
    return indir


def test_samples_without_a_lockstep_flag_group_as_lockstep_k(tmp_path, monkeypatch):
    calls = []
    _fake_samplers(monkeypatch, calls)
    indir, outdir = _inputs(tmp_path, {"a": (16, 12), "b": (20, 12)}), tmp_path / "out"
    INF.batch_sr_target_images(str(indir), str(outdir), None, seed=71, samples=3)
    assert calls == [("seeded", [(16, 12)] * 3, [71, 72, 73]), ("seeded", [(20, 12)] * 3, [71, 72, 73])]
    assert sorted(os.listdir(outdir)) == ["a_out.png", "a_out_s1.png", "a_out_s2.png", "b_out.png", "b_out_s1.png", "b_out_s2.png"]
    # skip-if-exists per output file: only the missing samples are drawn, each with its own seed
    os.remove(outdir / "a_out_s1.png")
    os.remove(outdir / "b_out.png")
    os.remove(outdir / "b_out_s2.png")
    calls.clear()
    INF.batch_sr_target_images(str(indir), str(outdir), None, seed=71, samples=3)
    assert calls == [("solo", [(16, 12)], 72), ("seeded", [(20, 12)] * 2, [71, 73])]
    # the default is today's run: one image per call with --seed
    calls.clear()
    INF.batch_sr_target_images(str(indir), str(tmp_path / "out1"), None, seed=71)
    assert calls == [("solo", [(16, 12)], 71), ("solo", [(20, 12)], 71)]


def test_samples_fill_lockstep_groups_and_count_against_the_tile_budget(tmp_path, monkeypatch):
    calls = []
    _fake_samplers(monkeypatch, calls)
    indir = _inputs(tmp_path, {"a": (64, 64), "b": (64, 64), "c": (120, 80)})      # x4: 1, 1 and 9 tiles per even step
    INF.batch_sr_target_images(str(indir), str(tmp_path / "o1"), None, seed=5, samples=2, lockstep=4)
    assert calls == [("seeded", [(64, 64)] * 4, [5, 6, 5, 6]), ("seeded", [(120, 80)] * 2, [5, 6])]
    calls.clear()
    INF.batch_sr_target_images(str(indir), str(tmp_path / "o2"), None, seed=5, samples=2, lockstep_tiles=12)
    # a x2, b x2 and the first copy of c are 1 + 1 + 1 + 1 + 9 = 13 > 12 tiles: the group closes before c; c's two copies are 18 > 12
    assert calls == [("seeded", [(64, 64)] * 4, [5, 6, 5, 6]), ("solo", [(120, 80)], 5), ("solo", [(120, 80)], 6)]


def test_new_entries_are_declared_in_both_headers():
    engine_h = open(os.path.join(ROOT, "include", "srgd_hip.h")).read()
    kernels_h = open(os.path.join(ROOT, "include", "srgd_hip_kernels.h")).read()
    assert re.search(r"\bint\s+srgd_sampler_noise_seeds\s*\(", engine_h)
    assert re.search(r"\bint\s+srgd_randn_streams\s*\(", kernels_h)
    from srgd_amd import _lib
    assert {"srgd_sampler_noise_seeds", "srgd_randn_streams"} <= set(_lib.PROTOTYPES)
