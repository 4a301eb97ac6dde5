"""``--reference_dir``, host side (no GPU): the yardstick itself (tests/metrics_cases.py) on hand-checkable cases, the two flags, the
pre-flight check of the references, ``metrics.json``'s layout, the way of the references through ``batch_sr_target_images`` into the
``sr_target_image*`` functions, the two C-ABI declarations and exports, the scratch formula and the resource table of the new
kernels."""
import inspect
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import _lib
from srgd_amd import inference as INF
from srgd_amd import metrics as MX
from tests import metrics_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")


def _argv(*extra):
    return ["-c", CONF, "-m", "ckpt.pth", "--input_dir", "in", "--output_dir", "out", *extra]


# ------------------------------------------------------------------------------------------- the restatement
def test_identical_images_give_inf_inf_one():
    out01, _ = M.pair(23, 27, 1)
    q = M.quantise(out01)
    for crop in (0, 4):
        got = M.restate(out01, q.astype(np.uint8), crop)
        assert got["psnr_y"] == math.inf and got["psnr_rgb"] == math.inf and abs(got["ssim_y"] - 1.0) <= 1e-12


def test_constant_offset_gives_the_closed_form_psnr():
    rng = np.random.default_rng(2)
    for d in (1, 3, 10):
        q = rng.integers(0, 256 - d, (20, 31, 3))
        got = M.restate_u8(q, (q + d).astype(np.uint8), 2)
        assert abs(got["psnr_rgb"] - 20.0 * math.log10(255.0 / d)) <= 1e-9
        # the luma of a grey offset d is d * (65.481 + 128.553 + 24.966) / 255
        assert abs(got["psnr_y"] - 20.0 * math.log10(255.0 / (d * 219.0 / 255.0))) <= 1e-9
        assert 0.0 < got["ssim_y"] < 1.0


def test_a_crop_that_removes_the_only_differing_pixels_gives_inf():
    out01, _ = M.pair(24, 30, 3)
    ref = M.quantise(out01).astype(np.uint8)
    ref[0, 5] ^= 255
    ref[20, 29] ^= 255
    ref[3, 3] ^= 255                                             # the last border row / column of a crop of 4
    inside = M.restate(out01, ref, 0)
    assert math.isfinite(inside["psnr_y"]) and math.isfinite(inside["psnr_rgb"]) and inside["ssim_y"] < 1.0
    cut = M.restate(out01, ref, 4)
    assert cut["psnr_y"] == math.inf and cut["psnr_rgb"] == math.inf and abs(cut["ssim_y"] - 1.0) <= 1e-12


def test_quantisation_is_the_fp32_product_truncated_and_non_finite_values_are_nan_inside_the_crop_only():
    k = np.arange(256, dtype=np.float32)
    vals = np.concatenate([k / np.float32(255.0), np.nextafter(k / np.float32(255.0), np.float32(2.0)),
                           np.nextafter(k / np.float32(255.0), np.float32(-1.0))])
    want = (vals.astype(np.float32) * np.float32(255.0)).astype(np.int64)
    got = M.quantise(np.broadcast_to(vals[None, None, :], (3, 1, vals.size)))
    assert np.array_equal(got[0, :, 0], want) and got.min() >= 0 and got.max() <= 255
    assert np.all(np.abs(want[:256] - np.arange(256)) <= 1) and np.all(want[512:] <= want[:256]) and np.all(want[256:512] >= want[:256])
    out01, ref = M.pair(19, 19, 4)
    bad = out01.copy()
    bad[1, 9, 9] = np.nan
    assert all(math.isnan(v) for v in M.restate(bad, ref, 4).values())
    edge = out01.copy()
    edge[1, 3, 9] = np.inf                                       # row 3: inside the 4-pixel border
    assert M.restate(edge, ref, 4) == M.restate(out01, ref, 4)
    assert all(math.isnan(v) for v in M.restate(edge, ref, 0).values())


def test_the_literal_2d_window_equals_its_separable_form_within_the_derived_bound():
    for (h, w, crop, kind) in ((23, 27, 0, "random"), (19, 19, 4, "random"), (40, 33, 4, "noisy")):
        out01, ref = (M.pair if kind == "random" else M.noisy_pair)(h, w, 5)
        lit, sep = M.restate(out01, ref, crop), M.restate(out01, ref, crop, ssim=M.ssim_separable)
        assert abs(lit["ssim_y"] - sep["ssim_y"]) <= M.TOL and lit["psnr_y"] == sep["psnr_y"]
    assert abs(M.window().sum() - 1.0) <= 1e-15 and M.window().shape == (11, 11)
    assert M.restate(*M.noisy_pair(40, 33, 5), 4)["ssim_y"] > 0.9                 # the high-SSIM regime it is meant to be


# ------------------------------------------------------------------------------------------- flags, pre-flight, metrics.json
def test_the_two_flags_parse(capsys):
    args = INF.parse_args(_argv())
    assert args.reference_dir is None and args.crop_border == 4
    args = INF.parse_args(_argv("--reference_dir", "gt", "--crop_border", "0", "--samples", "2", "--color_fix", "adain",
                                "--lockstep_tiles", "9"))
    assert args.reference_dir == "gt" and args.crop_border == 0 and args.samples == 2
    assert INF.parse_args(_argv("--reference_dir", "gt", "--lockstep", "3")).lockstep == 3
    with pytest.raises(SystemExit, match="crop_border"):
        INF.parse_args(_argv("--crop_border", "-1"))
    with pytest.raises(SystemExit):
        INF.parse_args(_argv("--crop_border", "four"))
    assert "--crop_border" in capsys.readouterr().err


def _png(path, w, h, seed=0):
    Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(path)


def test_the_preflight_check_names_missing_and_wrongly_sized_references(tmp_path):
    indir, gt = tmp_path / "in", tmp_path / "gt"
    indir.mkdir()
    gt.mkdir()
    for name, (w, h) in {"ok": (8, 6), "missing": (8, 6), "small": (8, 6), "swapped": (8, 6)}.items():
        _png(indir / f"{name}.png", w, h)
    (indir / "broken.png").write_bytes(b"not a png")             # the sampling loop reports and skips it: no reference asked for
    _png(gt / "ok.png", 32, 24)
    _png(gt / "small.png", 32, 23)
    _png(gt / "swapped.png", 24, 32)
    files = sorted(str(p) for p in indir.iterdir())
    problems = INF.reference_problems(files, str(gt))
    assert len(problems) == 3 and [p.split(":")[0] for p in problems] == ["missing.png", "small.png", "swapped.png"]
    assert "is missing" in problems[0] and "32x23" in problems[1] and "32x24" in problems[1] and "24x32" in problems[2]
    with pytest.raises(SystemExit) as err:
        INF.check_references(files, str(gt))
    assert err.value.code not in (0, None) and all(n in str(err.value.code) for n in ("missing.png", "small.png", "swapped.png"))
    assert "ok.png" not in str(err.value.code)
    # ... and batch_sr_target_images stops there, before any sampling (a None model would fail otherwise) and before any output
    with pytest.raises(SystemExit, match="missing.png"):
        INF.batch_sr_target_images(str(indir), str(tmp_path / "out"), None, reference_dir=str(gt))
    assert not list((tmp_path / "out").glob("*"))
    os.remove(indir / "missing.png"), os.remove(indir / "small.png"), os.remove(indir / "swapped.png")
    INF.check_references(sorted(str(p) for p in indir.iterdir()), str(gt))
    # a reference too small for an 11x11 window inside the crop is named too
    _png(indir / "tiny.png", 4, 4)
    _png(gt / "tiny.png", 16, 16)
    assert "11x11" in INF.reference_problems([str(indir / "tiny.png")], str(gt), crop_border=4)[0]
    assert INF.reference_problems([str(indir / "tiny.png")], str(gt), crop_border=2) == []


def test_metrics_document_means_and_non_finite_strings():
    rec = lambda a, b, c: {"psnr_y": a, "psnr_rgb": b, "ssim_y": c}          # noqa: E731
    rows = [("a.png", "a_out.png", rec(30.0, 28.0, 0.9)), ("a.png", "a_out_s1.png", rec(32.0, 29.0, 0.8)),
            ("b.png", "b_out.png", rec(math.inf, 20.0, math.nan)), ("b.png", "b_out_s1.png", rec(10.0, 22.0, 0.5))]
    doc = json.loads(json.dumps(INF.metrics_document(rows, 2, 4)))            # what is written is valid JSON
    assert doc["crop_border"] == 4 and list(doc["files"]) == ["a_out.png", "a_out_s1.png", "b_out.png", "b_out_s1.png"]
    assert doc["files"]["b_out.png"] == {"psnr_y": "inf", "psnr_rgb": 20.0, "ssim_y": "nan"}
    assert doc["images"]["a.png"] == {"psnr_y": 31.0, "psnr_rgb": 28.5, "ssim_y": (0.9 + 0.8) / 2}
    assert doc["images"]["b.png"] == {"psnr_y": "inf", "psnr_rgb": 21.0, "ssim_y": "nan"}
    assert doc["mean"] == {"psnr_y": "inf", "psnr_rgb": (28.5 + 21.0) / 2, "ssim_y": "nan"}
    single = INF.metrics_document(rows[:1] + rows[3:], 1, 0)
    assert "images" not in single and single["mean"]["psnr_y"] == 20.0 and single["crop_border"] == 0


def test_references_reach_the_samplers_and_metrics_json_is_written(tmp_path, monkeypatch):
    calls = []

    def fake(kind):
        def run(images, *a, **kw):
            ims = images if isinstance(images, list) else [images]
            outs = [Image.new("RGB", (im.size[0] * 4, im.size[1] * 4)) for im in ims]
            ret = outs if isinstance(images, list) else outs[0]
            if "reference" not in kw:
                calls.append((kind, len(ims), None, kw.get("crop_border", "absent")))
                return ret
            refs = kw["reference"] if isinstance(images, list) else [kw["reference"]]
            assert len(refs) == len(ims)
            for r, im in zip(refs, ims):
                assert r.dtype == torch.uint8 and tuple(r.shape) == (im.size[1] * 4, im.size[0] * 4, 3)
            calls.append((kind, len(ims), [int(r[0, 0, 0]) for r in refs], kw["crop_border"]))
            return ret, [{"psnr_y": float(r[0, 0, 0]), "psnr_rgb": 1.0, "ssim_y": 0.5} for r in refs]
        return run
    monkeypatch.setattr(INF, "sr_target_image", fake("solo"))
    monkeypatch.setattr(INF, "sr_target_images", fake("same"))
    monkeypatch.setattr(INF, "sr_target_images_mixed", fake("mixed"))
    monkeypatch.setattr(INF, "sr_target_images_seeded", fake("seeded"))
    indir, gt = tmp_path / "in", tmp_path / "gt"
    indir.mkdir()
    gt.mkdir()
    for i, (name, (w, h)) in enumerate({"a": (64, 64), "b": (64, 64), "c": (80, 64)}.items()):
        _png(indir / f"{name}.png", w, h)
        Image.fromarray(np.full((h * 4, w * 4, 3), 10 * (i + 1), dtype=np.uint8), "RGB").save(gt / f"{name}.png")
    run = lambda tag, **kw: INF.batch_sr_target_images(str(indir), str(tmp_path / tag), None, seed=71, **kw)   # noqa: E731
    run("solo", reference_dir=str(gt))
    assert calls == [("solo", 1, [10], 4), ("solo", 1, [20], 4), ("solo", 1, [30], 4)]
    doc = json.load(open(tmp_path / "solo" / "metrics.json"))
    assert list(doc["files"]) == ["a_out.png", "b_out.png", "c_out.png"] and "images" not in doc
    assert doc["files"]["b_out.png"] == {"psnr_y": 20.0, "psnr_rgb": 1.0, "ssim_y": 0.5} and doc["mean"]["psnr_y"] == 20.0
    calls.clear()
    run("same", reference_dir=str(gt), lockstep=2, crop_border=0)
    assert calls == [("same", 2, [10, 20], 0), ("solo", 1, [30], 0)]
    calls.clear()
    run("mixed", reference_dir=str(gt), lockstep_tiles=16, color_fix="wavelet")
    assert calls == [("mixed", 3, [10, 20, 30], 4)]
    calls.clear()
    run("seeded", reference_dir=str(gt), samples=2)              # the K samples of an image against the same reference
    assert calls == [("seeded", 2, [10, 10], 4), ("seeded", 2, [20, 20], 4), ("seeded", 2, [30, 30], 4)]
    doc = json.load(open(tmp_path / "seeded" / "metrics.json"))
    assert list(doc["files"]) == ["a_out.png", "a_out_s1.png", "b_out.png", "b_out_s1.png", "c_out.png", "c_out_s1.png"]
    assert list(doc["images"]) == ["a.png", "b.png", "c.png"] and doc["images"]["c.png"]["psnr_y"] == 30.0
    assert doc["mean"] == {"psnr_y": 20.0, "psnr_rgb": 1.0, "ssim_y": 0.5}
    # without the directory: no keyword, no file; a second run over existing outputs samples nothing and leaves the file alone
    calls.clear()
    run("plain", lockstep_tiles=16)
    run("plain2", samples=2)
    assert all(c[2] is None and c[3] == "absent" for c in calls) and len(calls) == 4
    assert not (tmp_path / "plain" / "metrics.json").exists() and not (tmp_path / "plain2" / "metrics.json").exists()
    before = open(tmp_path / "seeded" / "metrics.json").read()
    calls.clear()
    run("seeded", reference_dir=str(gt), samples=2)
    assert calls == [] and open(tmp_path / "seeded" / "metrics.json").read() == before


# ------------------------------------------------------------------------------------------- signatures, C ABI, resources
def test_tiled_sample_signatures_and_host_side_checks():
    from srgd_amd.model import ConditionalContinuousTimeGaussianDiffusionSR, ConditionalElucidatedDiffusionSR
    for cls in (ConditionalContinuousTimeGaussianDiffusionSR, ConditionalElucidatedDiffusionSR):
        params = inspect.signature(cls.tiled_sample).parameters
        assert params["reference"].default is None and params["crop_border"].default == 4
        assert "reference" not in inspect.signature(cls.sample).parameters            # the un-tiled path is out of scope
    for fn in (INF.sr_target_image, INF.sr_target_images, INF.sr_target_images_mixed, INF.sr_target_images_seeded):
        assert inspect.signature(fn).parameters["reference"].default is None
    assert inspect.signature(INF.batch_sr_target_images).parameters["reference_dir"].default is None
    assert INF.metrics_on_device is MX.metrics_on_device
    # the header's scratch formula: four doubles per 32x8 tile of the (h - 2 crop - 10) x (w - 2 crop - 10) positions
    assert MX.scratch_doubles([(19, 19)], 4) == 4 and MX.scratch_doubles([(19, 19)], 0) == 4 * 2
    assert MX.scratch_doubles([(26, 50), (27, 51)], 4) == 4 * 1 + 4 * 2 * 2
    assert MX.scratch_doubles([(300, 500)], 0) == 4 * 37 * 16 and MX.scratch_doubles([(1280, 1920)], 4) == 4 * 158 * 60
    for sizes, crop in (([(18, 40)], 4), ([(40, 18)], 4), ([(30, 30), (10, 30)], 0)):
        with pytest.raises(ValueError, match="11x11"):
            MX.scratch_doubles(sizes, crop)
        with pytest.raises(ValueError, match="11x11"):
            MX.metrics_on_device([torch.zeros(1, 3, h, w) for (h, w) in sizes],
                                 [torch.zeros(h, w, 3, dtype=torch.uint8) for (h, w) in sizes], crop)
    with pytest.raises(ValueError, match="crop_border"):
        MX.scratch_doubles([(30, 30)], -1)
    with pytest.raises(ValueError, match="references for"):
        MX.pack_references([torch.zeros(30, 30, 3, dtype=torch.uint8)], [(30, 30), (30, 30)], "cpu")
    with pytest.raises(ValueError, match="uint8"):
        MX.pack_references([torch.zeros(30, 31, 3, dtype=torch.uint8)], [(30, 30)], "cpu")
    with pytest.raises(ValueError, match="uint8"):
        MX.pack_references(torch.zeros(30, 30, 3), [(30, 30)], "cpu")
    flat, offs = MX.pack_references([torch.ones(12, 11, 3, dtype=torch.uint8), torch.zeros(11, 13, 3, dtype=torch.uint8)],
                                    [(12, 11), (11, 13)], "cpu")
    assert offs == [0, 396] and flat.numel() == 396 + 429 and int(flat.sum()) == 396


def test_entries_are_declared_prototyped_and_exported():
    # the metrics are a library of their own (libsrgd_metrics.so, include/srgd_metrics.h): the engine's export table stays as it is
    header = open(os.path.join(ROOT, "include", "srgd_metrics.h")).read()
    declared = set(re.findall(r"\b(srgd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == {"srgd_image_metrics", "srgd_image_metrics_images", "srgd_image_metrics_last_error"} == set(MX.PROTOTYPES)
    assert len(MX.PROTOTYPES["srgd_image_metrics"][1]) == 8 and len(MX.PROTOTYPES["srgd_image_metrics_images"][1]) == 10
    assert os.path.exists(MX.LIB_PATH), "build the library first (python -m srgd_amd.build)"
    nm = subprocess.run(["nm", "-D", "--defined-only", MX.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TtWw"}
    assert {n for n in exported if not n.startswith(("_init", "_fini", "__"))} == declared
    lib = MX.lib()                                        # binds every prototype
    assert lib.srgd_image_metrics_last_error() == b""
    assert not set(MX.PROTOTYPES) & set(_lib.PROTOTYPES)
    engine = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "srgd_image_metrics" not in engine


def test_metrics_kernels_do_not_spill_and_leave_room_for_two_workgroups_per_cu():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_table
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "metrics.hip")) if "metrics_" in r["name"]]
    assert sorted(r["name"] for r in rows) == ["metrics_finish_kernel", "metrics_tile_kernel"]
    for r in rows:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["lds"] <= 160 * 1024 // 2 and r["vgpr"] <= 128, r       # two 256-thread workgroups per CU: LDS and registers
