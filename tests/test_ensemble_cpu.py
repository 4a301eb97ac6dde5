"""``--ensemble``, host side (no GPU): the yardstick itself (tests/ensemble_cases.py) on hand-checkable cases, the flag, the output
names, ``ensemble.json``'s layout, ``metrics_document``'s new keyword, the grouping loop with fake samplers (two inputs, a resumed
run, a wrong-sized sample on disk, the mean images' way into ``metrics.json``), the C-ABI declarations and exports of the new
library, the scratch formula and the resource table of the new kernels."""
import inspect
import json
import math
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import _lib
from srgd_amd import ensemble as EN
from srgd_amd import inference as INF
from srgd_amd import metrics as MX
from tests import ensemble_cases as E
from tests.lib_exports import exports as _exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")


def _argv(*extra):
    return ["-c", CONF, "-m", "ckpt.pth", "--input_dir", "in", "--output_dir", "out", *extra]


# ------------------------------------------------------------------------------------------- the restatement
def test_identical_samples_give_the_sample_and_no_spread():
    one = E.random_samples(1, 9, 11, 3)[0]
    for k in (2, 3, 7, 256):
        mean, std, stats = E.restate(np.stack([one] * k))
        assert np.array_equal(mean, one) and not std.any() and stats == {"mean_std": 0.0, "max_std": 0.0}


def test_zero_and_255_give_mean_128_spread_255_and_max_std_127_5():
    x = np.zeros((2, 3, 5, 3), dtype=np.uint8)
    x[1] = 255
    mean, std, stats = E.restate(x)
    assert (mean == 128).all() and (std == 255).all() and stats == {"mean_std": 127.5, "max_std": 127.5}
    # halves go up in both outputs: {0, 1} has mean 0.5 -> 1 and 2 sigma = 1; {0, 0, 0, 1}: sigma = sqrt(3)/4, 2 sigma = 0.87 -> 1
    x = np.zeros((2, 1, 1, 3), dtype=np.uint8)
    x[1] = 1
    mean, std, stats = E.restate(x)
    assert (mean == 1).all() and (std == 1).all() and stats["max_std"] == 0.5
    x = np.zeros((4, 1, 1, 3), dtype=np.uint8)
    x[3] = 1
    mean, std, _ = E.restate(x)
    assert (mean == 0).all() and (std == 1).all()
    x = np.zeros((16, 1, 1, 3), dtype=np.uint8)                  # sigma = sqrt(15)/16 = 0.242: 2 sigma = 0.484 -> 0
    x[0] = 1
    assert not E.restate(x)[1].any()


@pytest.mark.parametrize("k", [2, 3, 5, 7, 64, 256])
def test_the_integer_spread_is_floor_of_two_sigma_plus_a_half_in_float64(k):
    x = E.random_samples(k, 24, 24, 100 + k)
    x[:, :8] = (x[:, :8] // 64) * 85                             # few levels: exact ties and small spreads appear too
    x[:, 8:12] = np.where(x[:, 8:12] > 127, 255, 0)
    _, _, _, d = E.sums(x)
    want = np.floor(2.0 * np.sqrt(d.astype(np.float64)) / k + 0.5).astype(np.int64)
    assert np.array_equal(E.spread_from_d(d, k).astype(np.int64), want)
    assert want.max() <= 255 and d.max() <= (k * k * 255 * 255) // 4
    mean = E.restate(x)[0].astype(np.float64)
    assert np.array_equal(mean, np.floor(x.astype(np.float64).sum(axis=0) / k + 0.5))


def test_mean01_truncates_back_to_the_mean_for_all_256_values():
    m = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    m01 = E.mean01(m)
    assert m01.dtype == np.float32 and m01.shape == (3, 16, 16)
    back = (m01 * np.float32(255.0)).astype(np.int64).transpose(1, 2, 0)          # unit_to_u8 / the metrics' quantisation
    assert np.array_equal(back, m.astype(np.int64))
    assert len(np.unique(E.restate(E.all_means_samples(5))[0])) == 256 and len(np.unique(E.restate(E.all_means_samples(2))[0])) == 256
    ext = E.restate(E.extreme_samples(3, 4, 4, 1))
    assert set(np.unique(ext[0])) <= {0, 85, 170, 255} and set(np.unique(ext[1])) <= {0, 240}    # 2 * 255 * sqrt(2) / 3 = 240.4


# ------------------------------------------------------------------------------------------- flag, names, documents
def test_the_flag_parses_and_needs_samples(capsys):
    assert INF.parse_args(_argv()).ensemble is False
    args = INF.parse_args(_argv("--samples", "3", "--ensemble", "--reference_dir", "gt", "--color_fix", "adain"))
    assert args.ensemble is True and args.samples == 3
    assert INF.parse_args(_argv("--ensemble", "--samples", "2", "--lockstep_tiles", "9")).ensemble is True
    for extra in ((), ("--samples", "1"), ("--samples", "257")):
        with pytest.raises(SystemExit, match="--ensemble"):
            INF.parse_args(_argv("--ensemble", *extra))
    params = inspect.signature(INF.batch_sr_target_images).parameters
    assert params["ensemble"].default is False and params["ensemble_name"].default == "ensemble.json"
    assert INF.ensemble_on_device is EN.ensemble_on_device


def test_ensemble_output_names():
    assert INF.ensemble_output_names("/data/in/a.png") == ("a_out_mean.png", "a_out_std.png")
    assert INF.ensemble_output_names("b_c.png") == ("b_c_out_mean.png", "b_c_out_std.png")
    names = {INF.sample_output_name("a.png", k) for k in range(12)}
    assert not names & set(INF.ensemble_output_names("a.png"))


def test_ensemble_document():
    rows = [("a.png", "a_out_mean.png", "a_out_std.png", {"mean_std": 2.0, "max_std": 30.5}),
            ("b.png", "b_out_mean.png", "b_out_std.png", {"mean_std": 4.0, "max_std": 127.5})]
    doc = json.loads(json.dumps(INF.ensemble_document(rows, 5)))
    assert doc == {"samples": 5, "mean_std": 3.0,
                   "files": {"a.png": {"mean": "a_out_mean.png", "std": "a_out_std.png", "mean_std": 2.0, "max_std": 30.5},
                             "b.png": {"mean": "b_out_mean.png", "std": "b_out_std.png", "mean_std": 4.0, "max_std": 127.5}}}
    assert list(doc) == ["samples", "files", "mean_std"]


def test_metrics_document_is_unchanged_without_the_keyword_and_gains_two_keys_with_it():
    rec = lambda a, b, c: {"psnr_y": a, "psnr_rgb": b, "ssim_y": c}          # noqa: E731
    rows = [("a.png", "a_out.png", rec(30.0, 28.0, 0.9)), ("a.png", "a_out_s1.png", rec(32.0, 29.0, 0.8)),
            ("b.png", "b_out.png", rec(20.0, 20.0, 0.5)), ("b.png", "b_out_s1.png", rec(10.0, 22.0, 0.5))]
    plain = INF.metrics_document(rows, 2, 4)
    assert list(plain) == ["crop_border", "files", "images", "mean"]
    assert inspect.signature(INF.metrics_document).parameters["ensemble"].default is None
    assert json.dumps(INF.metrics_document(rows, 2, 4, ensemble=None)) == json.dumps(plain)
    assert json.dumps(INF.metrics_document(rows, 2, 4, ensemble=[])) == json.dumps(plain)
    doc = INF.metrics_document(rows, 2, 4, ensemble=[("a.png", rec(33.0, 30.0, 0.95)), ("b.png", rec(math.inf, 24.0, 0.55))])
    assert list(doc) == ["crop_border", "files", "images", "mean", "ensemble", "ensemble_mean"]
    assert {k: doc[k] for k in plain} == plain
    assert doc["ensemble"] == {"a.png": rec(33.0, 30.0, 0.95), "b.png": {"psnr_y": "inf", "psnr_rgb": 24.0, "ssim_y": 0.55}}
    assert doc["ensemble_mean"] == {"psnr_y": "inf", "psnr_rgb": 27.0, "ssim_y": 0.75}


# ------------------------------------------------------------------------------------------- the grouping loop
def _fake_sample(size, seed):
    """The x4 'sample' of an input of ``size`` (w, h) for a noise seed: reproducible, different per seed."""
    w, h = size
    return Image.fromarray(np.random.default_rng([seed, w, h]).integers(0, 256, (h * 4, w * 4, 3), dtype=np.uint8), "RGB")


def _fake_samplers(monkeypatch, calls):
    def fake(kind):
        def run(images, *a, **kw):
            ims = images if isinstance(images, list) else [images]
            seeds = list(a[0]) if kind == "seeded" else [kw.get("seed")] * len(ims)
            calls.append((kind, [im.size for im in ims], seeds))
            outs = [_fake_sample(im.size, s) for im, s in zip(ims, seeds)]
            ret = outs if isinstance(images, list) else outs[0]
            if "reference" not in kw:
                return ret
            refs = kw["reference"] if isinstance(images, list) else [kw["reference"]]
            return ret, [{"psnr_y": 20.0 + s - 71, "psnr_rgb": 1.0, "ssim_y": 0.5} for s, _ in zip(seeds, refs)]
        return run
    monkeypatch.setattr(INF, "sr_target_image", fake("solo"))
    monkeypatch.setattr(INF, "sr_target_images", fake("same"))
    monkeypatch.setattr(INF, "sr_target_images_mixed", fake("mixed"))
    monkeypatch.setattr(INF, "sr_target_images_seeded", fake("seeded"))


def _fake_ensemble(monkeypatch, batches):
    """``ensemble_on_device`` replaced by the yardstick; ``batches`` records the sizes of every batched call."""
    def run(samples, return_mean01=False):
        assert isinstance(samples, list) and all(t.dtype == torch.uint8 and t.dim() == 4 for t in samples)
        batches.append([tuple(t.shape) for t in samples])
        out = []
        for t in samples:
            mean, std, stats = E.restate(t.numpy())
            item = (torch.from_numpy(mean), torch.from_numpy(std), stats)
            out.append(item + (torch.from_numpy(E.mean01(mean))[None],) if return_mean01 else item)
        return out
    monkeypatch.setattr(INF, "ensemble_on_device", run)


def _inputs(tmp_path, sizes):
    indir = tmp_path / "in"
    indir.mkdir()
    rng = np.random.default_rng(0)
    for name, (w, h) in sizes.items():
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(indir / f"{name}.png")
    return indir


def _png(path):
    return np.asarray(Image.open(path).convert("RGB"))


def test_two_inputs_three_samples_a_resumed_run_and_a_wrong_sized_sample(tmp_path, monkeypatch, capsys):
    calls, batches = [], []
    _fake_samplers(monkeypatch, calls)
    _fake_ensemble(monkeypatch, batches)
    indir, outdir = _inputs(tmp_path, {"a": (6, 5), "b": (7, 5)}), tmp_path / "out"
    run = lambda **kw: INF.batch_sr_target_images(str(indir), str(outdir), None, seed=71, samples=3, ensemble=True, **kw)  # noqa: E731
    run()
    assert calls == [("seeded", [(6, 5)] * 3, [71, 72, 73]), ("seeded", [(7, 5)] * 3, [71, 72, 73])]
    assert batches == [[(3, 20, 24, 3)], [(3, 20, 28, 3)]]       # the files one flush() completes go into one call
    assert sorted(os.listdir(outdir)) == sorted([f"{n}_out{s}.png" for n in "ab" for s in ("", "_s1", "_s2", "_mean", "_std")]
                                                + ["ensemble.json"])
    doc = json.load(open(outdir / "ensemble.json"))
    assert doc["samples"] == 3 and list(doc["files"]) == ["a.png", "b.png"]
    for name in "ab":
        stack = np.stack([_png(outdir / INF.sample_output_name(f"{name}.png", k)) for k in range(3)])
        mean, std, stats = E.restate(stack)
        assert np.array_equal(_png(outdir / f"{name}_out_mean.png"), mean) and np.array_equal(_png(outdir / f"{name}_out_std.png"), std)
        assert doc["files"][f"{name}.png"] == {"mean": f"{name}_out_mean.png", "std": f"{name}_out_std.png", **stats}
    assert doc["mean_std"] == (doc["files"]["a.png"]["mean_std"] + doc["files"]["b.png"]["mean_std"]) / 2
    assert not (outdir / "metrics.json").exists()
    # a second run over complete outputs: nothing sampled, nothing decoded, nothing rewritten
    before = {n: open(outdir / n, "rb").read() for n in os.listdir(outdir)}
    calls.clear(), batches.clear()
    run()
    assert calls == [] and batches == [] and {n: open(outdir / n, "rb").read() for n in os.listdir(outdir)} == before
    # resumed run: one sample and both ensemble files of `a` are gone - only that sample is drawn, the other two are read from disk
    for n in ("a_out_s1.png", "a_out_mean.png", "a_out_std.png"):
        os.remove(outdir / n)
    run()
    assert calls == [("solo", [(6, 5)], [72])] and batches == [[(3, 20, 24, 3)]]
    after = {n: open(outdir / n, "rb").read() for n in os.listdir(outdir)}
    assert {n: v for n, v in after.items() if n != "ensemble.json"} == {n: v for n, v in before.items() if n != "ensemble.json"}
    doc2 = json.load(open(outdir / "ensemble.json"))
    assert doc2["files"] == {"a.png": doc["files"]["a.png"]}     # the files whose ensemble this run took
    # every sample on disk, only the ensemble files missing: both files of both inputs in ONE batched call, nothing sampled
    for n in ("a_out_mean.png", "b_out_std.png"):
        os.remove(outdir / n)
    calls.clear(), batches.clear()
    run()
    assert calls == [] and batches == [[(3, 20, 24, 3), (3, 20, 28, 3)]]
    assert {n: open(outdir / n, "rb").read() for n in os.listdir(outdir) if n != "ensemble.json"} \
        == {n: v for n, v in before.items() if n != "ensemble.json"}
    assert json.load(open(outdir / "ensemble.json")) == doc
    # a wrong-sized sample on disk: reported by name, that file's ensemble is skipped, the run goes on with the other file
    Image.new("RGB", (8, 8)).save(outdir / "a_out_s2.png")
    for n in ("a_out.png", "a_out_mean.png", "a_out_std.png", "b_out_mean.png", "b_out_std.png"):
        os.remove(outdir / n)
    calls.clear(), batches.clear()
    capsys.readouterr()
    run()
    said = capsys.readouterr().out
    assert "a_out_s2.png" in said and "8x8" in said and "24x20" in said and "no ensemble for a.png" in said
    assert calls == [("solo", [(6, 5)], [71])] and batches == [[(3, 20, 28, 3)]]
    assert not (outdir / "a_out_mean.png").exists() and not (outdir / "a_out_std.png").exists()
    assert open(outdir / "b_out_mean.png", "rb").read() == before["b_out_mean.png"]
    assert list(json.load(open(outdir / "ensemble.json"))["files"]) == ["b.png"]


def test_lockstep_groups_smaller_and_larger_than_k_and_the_reference_dir(tmp_path, monkeypatch):
    calls, batches, scored = [], [], []
    _fake_samplers(monkeypatch, calls)
    _fake_ensemble(monkeypatch, batches)

    def fake_metrics(outs, refs, crop_border=4):
        assert all(tuple(o.shape) == (1, 3, r.shape[0], r.shape[1]) and o.dtype == torch.float32 for o, r in zip(outs, refs))
        scored.append((len(outs), crop_border))
        return [{"psnr_y": float(r[0, 0, 0]), "psnr_rgb": 2.0, "ssim_y": 0.25} for r in refs]
    monkeypatch.setattr(INF, "metrics_on_device", fake_metrics)
    indir, gt = _inputs(tmp_path, {"a": (64, 64), "b": (64, 64), "c": (64, 64)}), tmp_path / "gt"
    gt.mkdir()
    for i, name in enumerate("abc"):
        Image.fromarray(np.full((256, 256, 3), 10 * (i + 1), dtype=np.uint8), "RGB").save(gt / f"{name}.png")
    run = lambda tag, **kw: INF.batch_sr_target_images(str(indir), str(tmp_path / tag), None, seed=71, samples=2, ensemble=True,  # noqa: E731
                                                       **kw)
    run("two")                                                   # groups of K: a file per flush
    assert batches == [[(2, 256, 256, 3)]] * 3
    batches.clear()
    run("three", lockstep=3)                                     # a a b | b c c: the second flush completes b and c
    assert batches == [[(2, 256, 256, 3)], [(2, 256, 256, 3)] * 2]
    batches.clear()
    run("one", lockstep_tiles=1)                                 # every sample alone
    assert batches == [[(2, 256, 256, 3)]] * 3 and [c[0] for c in calls[-6:]] == ["solo"] * 6
    for tag in ("three", "one"):
        for n in os.listdir(tmp_path / "two"):
            assert open(tmp_path / tag / n, "rb").read() == open(tmp_path / "two" / n, "rb").read(), (tag, n)
    run("gt", reference_dir=str(gt), crop_border=2, lockstep=6)
    assert scored == [(3, 2)]
    doc = json.load(open(tmp_path / "gt" / "metrics.json"))
    assert list(doc) == ["crop_border", "files", "images", "mean", "ensemble", "ensemble_mean"]
    assert doc["ensemble"] == {f"{n}.png": {"psnr_y": 10.0 * (i + 1), "psnr_rgb": 2.0, "ssim_y": 0.25} for i, n in enumerate("abc")}
    assert doc["ensemble_mean"] == {"psnr_y": 20.0, "psnr_rgb": 2.0, "ssim_y": 0.25}
    assert open(tmp_path / "gt" / "ensemble.json").read() == open(tmp_path / "two" / "ensemble.json").read()
    # without --ensemble: no call, no file, today's metrics.json
    batches.clear()
    INF.batch_sr_target_images(str(indir), str(tmp_path / "plain"), None, seed=71, samples=2, reference_dir=str(gt), crop_border=2)
    plain = json.load(open(tmp_path / "plain" / "metrics.json"))
    assert batches == [] and not (tmp_path / "plain" / "ensemble.json").exists() and list(plain) == ["crop_border", "files", "images", "mean"]
    assert plain == {k: doc[k] for k in plain} and len(os.listdir(tmp_path / "plain")) == 7
    with pytest.raises(ValueError, match="samples"):
        INF.batch_sr_target_images(str(indir), str(tmp_path / "bad"), None, seed=71, samples=1, ensemble=True)


# ------------------------------------------------------------------------------------------- Python-side checks, C ABI, resources
def test_host_side_checks_of_the_module():
    assert EN.padded(105) == 112 and EN.padded(768) == 768 and EN.padded(3) == 16 and EN.VEC == E.VEC and EN.CHUNK == E.CHUNK
    # the header's scratch formula: two 8-byte words per chunk of 4096 elements
    assert EN.scratch_doubles([(1, 1)]) == 2 and EN.scratch_doubles([(32, 32)]) == 2 and EN.scratch_doubles([(37, 37)]) == 4
    assert EN.scratch_doubles([(64, 64), (5, 7)]) == 6 + 2 and EN.scratch_doubles([(1280, 1920)]) == 2 * 1800
    with pytest.raises(ValueError, match="size"):
        EN.scratch_doubles([(0, 4)])
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)               # noqa: E731
    for bad in (u8(3, 4, 4), u8(2, 4, 4, 4), torch.zeros(2, 4, 4, 3), [], [u8(2, 4, 4, 3), u8(3, 4, 4, 3)], u8(1, 4, 4, 3),
                u8(257, 1, 1, 3), [u8(2, 4, 4, 3), "x"], None, u8(2, 0, 4, 3)):
        with pytest.raises(ValueError, match="ensemble_on_device"):
            EN.ensemble_on_device(bad)
    with pytest.raises(_lib.SrgdHipError, match="no CPU fallback"):            # a missing GPU is an error, never another path
        EN.ensemble_on_device(u8(2, 4, 4, 3))
    for fn in ("ensemble_flat", "ensemble_flat_device"):
        assert list(inspect.signature(getattr(EN, fn)).parameters) == ["samples", "sample_offsets", "sizes", "n_samples", "mean_u8", "std_u8",
                                                                        "out_offsets", "mean01", "mean01_offsets"]


def test_entries_are_declared_prototyped_and_exported_by_a_library_of_their_own():
    header = open(os.path.join(ROOT, "include", "srgd_ensemble.h")).read()
    declared = set(re.findall(r"\b(srgd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == {"srgd_image_ensemble", "srgd_image_ensemble_images", "srgd_image_ensemble_last_error"} == set(EN.PROTOTYPES)
    # the number of parameters of every declaration is the number of ctypes argument types
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, (_, argtypes) in EN.PROTOTYPES.items():
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", flat).group(1).strip()
        assert (0 if params == "void" else len(params.split(","))) == len(argtypes), name
    assert os.path.exists(EN.LIB_PATH), "build the library first (python -m srgd_amd.build)"
    assert _exports(EN.LIB_PATH) == declared
    lib = EN.lib()                                        # binds every prototype
    assert lib.srgd_image_ensemble_last_error() == b""
    # it exports nothing that either of the other two libraries exports, and they export nothing of it
    assert not declared & _exports(_lib.LIB_PATH) and not declared & _exports(MX.LIB_PATH)
    assert not set(EN.PROTOTYPES) & set(_lib.PROTOTYPES) and not set(EN.PROTOTYPES) & set(MX.PROTOTYPES)
    assert not any("ensemble" in n for n in _exports(_lib.LIB_PATH) | _exports(MX.LIB_PATH))
    # the definition's wording is fixed in the header
    for phrase in ("D = K*Q - S^2", "m = (2*S + K) div (2*K)", "(2s-1)^2 * K^2 <= 16*D < (2s+1)^2 * K^2", "s = 0 if 16*D < K^2",
                   "(float)m / 255.0f", "mean_std = (sum_e sqrt((double)D_e) / K) / (3*h*w)", "max_std = sqrt((double)max_e D_e) / K",
                   "16 * ceil(3*h*w / 4096) bytes"):
        assert phrase in header, phrase


def test_refusals_need_no_gpu():
    # every refusal is decided on the host before anything is launched, so it can be checked here: -1 and a message
    lib = EN.lib()
    import ctypes as C
    off, hw = (C.c_int64 * 1)(0), (C.c_int32 * 2)(4, 4)
    p = C.c_void_p(4096)                                   # never dereferenced: a refused call launches nothing
    ok = dict(samples=p, offs=off, hw=hw, n=1, k=3, mean=p, std=p, out=off, m01=None, m01_offs=None, stats=p, scratch=p)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.srgd_image_ensemble_images(a["samples"], a["offs"], a["hw"], a["n"], a["k"], a["mean"], a["std"], a["out"], a["m01"],
                                            a["m01_offs"], a["stats"], a["scratch"], None)
        return rc, lib.srgd_image_ensemble_last_error().decode()
    cases = {"null": [dict(samples=None), dict(offs=None), dict(hw=None), dict(mean=None), dict(std=None), dict(out=None),
                      dict(stats=None), dict(scratch=None)],
             "together": [dict(m01=p), dict(m01_offs=off)],
             "n_images": [dict(n=0), dict(n=-1)],
             "n_samples": [dict(k=1), dict(k=257), dict(k=0)],
             "bad size": [dict(hw=(C.c_int32 * 2)(0, 4)), dict(hw=(C.c_int32 * 2)(4, -1))],
             "2^31 - 256": [dict(hw=(C.c_int32 * 2)(26755, 26755)), dict(hw=(C.c_int32 * 2)(1, 715827798))],
             "misaligned offset": [dict(offs=(C.c_int64 * 1)(8)), dict(out=(C.c_int64 * 1)(17))],
             "offset outside": [dict(offs=(C.c_int64 * 1)(-16)), dict(out=(C.c_int64 * 1)(1 << 36))],
             "16-byte aligned": [dict(samples=C.c_void_p(4100)), dict(mean=C.c_void_p(4104)), dict(std=C.c_void_p(4097))],
             "8-byte aligned": [dict(stats=C.c_void_p(4100)), dict(scratch=C.c_void_p(4100))]}
    for word, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == -1 and word in msg and msg.startswith("srgd_image_ensemble_images: "), (kw, msg)
    rc = lib.srgd_image_ensemble(p, 1, 4, 4, p, p, None, p, p, None)
    assert rc == -1 and lib.srgd_image_ensemble_last_error().decode().startswith("srgd_image_ensemble: ")
    assert 3 * 715827798 == 2 ** 31 - 254 and 3 * 715827797 < 2 ** 31 - 256 <= 3 * 715827798       # the first refused element count


def test_ensemble_kernels_do_not_spill_and_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_table
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "ensemble.hip")) if "ensemble_" in r["name"]]
    assert sorted(r["name"] for r in rows) == ["ensemble_finish_kernel", "ensemble_kernel"]
    for r in rows:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["lds"] <= 160 * 1024 // 4 and r["vgpr"] <= 128, r       # four 256-thread workgroups per CU: LDS and registers
