"""``--color_fix``, host side (no GPU): the flag, its way by keyword through ``batch_sr_target_images`` into each of the four
``sr_target_image*`` functions, the two C-ABI declarations and exports, the no-spill table of the new kernels, and the yardstick
itself (tests/color_fix_cases.py: the literal restatement against its one-chain separable form)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import _lib
from srgd_amd import inference as INF
from tests import color_fix_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")


def _argv(*extra):
    return ["-c", CONF, "-m", "ckpt.pth", "--input_dir", "in", "--output_dir", "out", *extra]


def test_color_fix_flag_default_and_choices(capsys):
    assert INF.parse_args(_argv()).color_fix == "none"
    for mode in ("none", "wavelet", "adain"):
        assert INF.parse_args(_argv("--color_fix", mode)).color_fix == mode
    assert INF.parse_args(_argv("--color_fix", "adain", "--samples", "2", "--lockstep_tiles", "9")).samples == 2
    with pytest.raises(SystemExit):
        INF.parse_args(_argv("--color_fix", "histogram"))
    assert "--color_fix" in capsys.readouterr().err


def _fake_samplers(monkeypatch, calls):
    def fake(kind):
        def run(images, *a, **kw):
            ims = images if isinstance(images, list) else [images]
            calls.append((kind, len(ims), kw.get("color_fix", "absent")))
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


def test_the_keyword_reaches_each_of_the_four_samplers(tmp_path, monkeypatch):
    calls = []
    _fake_samplers(monkeypatch, calls)
    indir = _inputs(tmp_path, {"a": (64, 64), "b": (64, 64), "c": (80, 64)})
    run = lambda tag, **kw: INF.batch_sr_target_images(str(indir), str(tmp_path / tag), None, seed=71, **kw)   # noqa: E731
    run("solo", color_fix="wavelet")
    assert calls == [("solo", 1, "wavelet")] * 3
    calls.clear()
    run("same", color_fix="adain", lockstep=2)
    assert calls == [("same", 2, "adain"), ("solo", 1, "adain")]
    calls.clear()
    run("mixed", color_fix="wavelet", lockstep_tiles=16)
    assert calls == [("mixed", 3, "wavelet")]
    calls.clear()
    run("seeded", color_fix="adain", samples=2)                  # every sample of an image with the same mode
    assert calls == [("seeded", 2, "adain")] * 3
    # a run without the flag (and one with --color_fix none) hands on nothing but None / "none"
    for tag, kw in (("d1", {}), ("d2", {"color_fix": "none"}), ("d3", {"color_fix": None})):
        calls.clear()
        run(tag, lockstep_tiles=16, **kw)
        run(tag + "s", samples=2, **kw)
        run(tag + "l", lockstep=2, **kw)
        assert len(calls) == 6 and {c[0] for c in calls} == {"mixed", "seeded", "same", "solo"}
        assert all(c[2] in (None, "none", "absent") for c in calls), calls


def test_the_samplers_hand_the_mode_to_tiled_sample(monkeypatch):
    seen = []

    class FakeModel:
        device = torch.device("cpu")

        def tiled_sample(self, **kw):
            seen.append(kw.get("color_fix", "absent"))
            c = kw["condition_x"]
            return [torch.zeros_like(x) for x in c] if isinstance(c, list) else torch.zeros_like(c)

    monkeypatch.setattr(INF, "upsample_bicubic_on_device", lambda im, scale, dev: torch.zeros(1, 3, im.size[1] * scale, im.size[0] * scale))
    monkeypatch.setattr(INF, "unit_tensor_to_pil_on_device", lambda t: Image.new("RGB", (t.shape[-1], t.shape[-2])))
    im = Image.new("RGB", (8, 6))
    model = FakeModel()
    for mode, want in (("wavelet", "wavelet"), ("adain", "adain"), (None, None), ("none", None)):
        seen.clear()
        kw = {} if mode is None else {"color_fix": mode}
        INF.sr_target_image(im, model, test_label=None, **kw)
        INF.sr_target_images([im, im], model, test_label=None, **kw)
        INF.sr_target_images_mixed([im, im], model, test_label=None, **kw)
        INF.sr_target_images_seeded([im, im], [1, 2], model, test_label=None, **kw)
        assert len(seen) == 4
        assert all(s == want for s in seen) if want else all(s in (None, "none", "absent") for s in seen), (mode, seen)
    for fn in (INF.sr_target_image, INF.sr_target_images, INF.sr_target_images_mixed, INF.sr_target_images_seeded,
               INF.batch_sr_target_images):
        assert inspect.signature(fn).parameters["color_fix"].default is None


def test_tiled_sample_signatures_and_mode_check():
    from srgd_amd.colorfix import check_mode, scratch_elements
    from srgd_amd.model import ConditionalContinuousTimeGaussianDiffusionSR, ConditionalElucidatedDiffusionSR
    for cls in (ConditionalContinuousTimeGaussianDiffusionSR, ConditionalElucidatedDiffusionSR):
        assert inspect.signature(cls.tiled_sample).parameters["color_fix"].default is None
        assert "color_fix" not in inspect.signature(cls.sample).parameters          # the un-tiled path is out of scope
    assert check_mode(None) is None and check_mode("none") is None and check_mode("adain") == "adain"
    with pytest.raises(ValueError, match="mode"):
        check_mode("histogram")
    with pytest.raises(ValueError, match="mode"):
        INF.color_fix_on_device(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4), "histogram")
    # the header's scratch formulas
    assert scratch_elements("wavelet", [0], [(5, 7)]) == 2 * 108                    # 3*5*7 = 105 -> 108
    assert scratch_elements("wavelet", [1, 200], [(5, 7), (2, 3)]) == 2 * 220       # extent 218 -> 220
    assert scratch_elements("adain", [0, 0], [(64, 64), (64, 65)]) * 4 == 96 * 2 + 96 * 3


def test_entries_are_declared_prototyped_and_exported():
    header = open(os.path.join(ROOT, "include", "srgd_hip.h")).read()
    names = ["srgd_image_color_fix", "srgd_image_color_fix_images"]
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["srgd_image_color_fix"][1]) == 8 and len(_lib.PROTOTYPES["srgd_image_color_fix_images"][1]) == 9
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m srgd_amd.build)"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert set(names) <= exported
    assert len([n for n in exported if n.startswith("srgd_")]) == len(_lib.PROTOTYPES) == 58


def test_color_fix_kernels_do_not_spill():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_table
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "imageio.hip"))
            if "wavelet_pass_kernel" in r["name"] or "adain_" in r["name"]]
    assert len(rows) == 7, [r["name"] for r in rows]               # four wavelet instances, three adain kernels
    for r in rows:
        assert r["spill"] == 0 and r["scratch"] == 0, r


@pytest.mark.parametrize("size", K.SIZES)
def test_the_literal_restatement_equals_its_one_chain_separable_form(size):
    c, s = K.pair(size[0], size[1], 9, "wavelet")
    lit, chain = K.wavelet_literal(c, s), K.wavelet_one_chain(c, s)
    assert lit.dtype == torch.float64 and float((lit - chain).abs().max()) == 0.0
    assert float(lit.min()) < 0.0 and float(lit.max()) > 1.0        # before the clamp the values leave [0,1]
    # in fp32 the chain stays within 22 roundings of the float64 value
    assert float((K.wavelet_one_chain(c, s, torch.float32).double() - lit).abs().max()) <= 2e-6
    # adain: the restatement against plain formulas on one channel
    ca, sa = K.pair(size[0], size[1], 9, "adain")
    got = K.adain_literal(ca, sa)
    x, y = ca[1].double(), sa[1].double()
    want = (x - x.mean()) / (x.var(unbiased=True) + 1e-5).sqrt() * (y.var(unbiased=True) + 1e-5).sqrt() + y.mean()
    assert float((got[1] - want).abs().max()) <= 1e-14
