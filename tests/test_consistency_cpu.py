"""``--consistency``, host side (no GPU): the yardstick itself (tests/consistency_cases.py: Pillow, its restatement, the overshoot
input), the five coefficient vectors of the library against Pillow's formula, the five-vector fact the kernel rests on, the C-ABI
declarations, exports and refusals of the new library, the resource table of the new kernels, the flag, ``consistency.json``'s layout
and the batch loop with fake samplers and a fake ``consistency_on_device``."""
import ctypes as C
import inspect
import json
import math
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import pil_resample as PR
from srgd_amd import _lib
from srgd_amd import consistency as CS
from srgd_amd import ensemble as EN
from srgd_amd import inference as INF
from srgd_amd import metrics as MX
from tests import consistency_cases as K
from tests import ensemble_cases as E
from tests.lib_exports import exports as _exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")
ENTRIES = {"srgd_image_consistency", "srgd_image_consistency_images", "srgd_image_consistency_coeffs", "srgd_image_consistency_last_error"}


def _argv(*extra):
    return ["-c", CONF, "-m", "ckpt.pth", "--input_dir", "in", "--output_dir", "out", *extra]


# ------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("h,w", K.SIZES)
def test_the_restatement_equals_pillow_and_the_oracle(h, w):
    for out in (K.random_pair(h, w, 1)[0], K.overshoot_output(h, w), K.pillow_up(K.random_pair(h, w, 2)[1])):
        down = K.pillow_down(out)
        assert down.shape == (h, w, 3) and down.dtype == np.uint8
        assert np.array_equal(K.restate(out)[0], down)
        assert np.array_equal(PR.resize_bicubic_u8(out, h, w), down)


@pytest.mark.parametrize("h,w", K.OVERSHOOT_SIZES)
def test_the_overshoot_input_drives_accumulators_past_both_ends_in_both_passes(h, w):
    out = K.overshoot_output(h, w)
    assert set(np.unique(out)) == {0, 255}
    _, counts = K.restate(out)
    for name in ("h", "v"):
        below, above = counts[name]
        assert below > 0 and above > 0, (name, counts)           # the clip is really exercised, both ways, in both passes
    # block edges on every phase of 4 (first row, channel 0)
    edges = np.flatnonzero(np.diff(out[0, :, 0].astype(np.int64)) != 0) + 1
    assert len(edges) < 4 or {int(e) % 4 for e in edges} == {0, 1, 2, 3}


def test_the_three_numbers_of_hand_checkable_cases():
    assert K.record((0, 0, 0, 0), 5, 7) == {"lr_psnr": math.inf, "lr_mse": 0.0, "lr_max_abs": 0.0}
    rec = K.record((255 * 255 * 35,) * 3 + (255,), 5, 7)
    assert rec == {"lr_psnr": 0.0, "lr_mse": 65025.0, "lr_max_abs": 255.0}
    assert K.record((3, 0, 0, 1), 1, 1)["lr_mse"] == 1.0 and abs(K.record((3, 0, 0, 1), 1, 1)["lr_psnr"] - 48.1308036086791) < 1e-12
    assert CS.record(3, 0, 0, 1, 1, 1) == K.record((3, 0, 0, 1), 1, 1) and CS.record(0, 0, 0, 0, 5, 7) == K.record((0, 0, 0, 0), 5, 7)
    # a constant output reduces to the same constant (every coefficient row sums to 1 << 22): consistent with the constant input
    for v in (0, 1, 128, 255):
        down, ints, rec = K.yardstick(K.constant(20, 28, v), K.constant(5, 7, v))
        assert (down == v).all() and ints == (0, 0, 0, 0) and rec["lr_psnr"] == math.inf
    # O = Pillow x4 of L is consistent with L up to the rounding of the two resamplings, not exactly
    lr = K.random_pair(16, 33, 3)[1]
    _, ints, rec = K.yardstick(K.pillow_up(lr), lr)
    assert 0 < rec["lr_mse"] < K.yardstick(*K.random_pair(16, 33, 3))[2]["lr_mse"]


# ------------------------------------------------------------------------------------------- coefficients
def test_the_librarys_five_vectors_are_pillows_rows():
    got = CS.coeffs()
    bounds, kk = PR.precompute_coeffs(256, 64)
    assert kk.shape == (64, 17) and not kk[:, 16].any()
    for vec, row in zip(got, (0, 1, 10, 62, 63)):
        assert vec == kk[row, :16].tolist(), row
    assert [int(bounds[r, 1]) for r in (0, 1, 10, 62, 63)] == [10, 14, 16, 14, 10]
    assert sum(got[2]) == 1 << 22 and got[2] == got[2][::-1]
    assert max(abs(v) for vec in got for v in vec) < 1 << 23     # a tap is a 24-bit multiply in the kernel
    assert CS.lib().srgd_image_consistency_coeffs(None) == -1
    assert CS.lib().srgd_image_consistency_last_error().decode().startswith("srgd_image_consistency_coeffs: ")


@pytest.mark.parametrize("n", list(range(5, 70)) + [100, 257])
def test_the_five_vector_fact(n):
    five = np.array(CS.coeffs(), dtype=np.int64)
    bounds, kk = PR.precompute_coeffs(4 * n, n)
    kk = kk.astype(np.int64)
    assert not kk[:, 16:].any()
    assert bounds[0].tolist() == [0, 10] and bounds[1].tolist() == [0, 14]
    assert bounds[n - 2].tolist() == [4 * n - 14, 14] and bounds[n - 1].tolist() == [4 * n - 10, 10]
    assert np.array_equal(kk[0, :16], five[0]) and np.array_equal(kk[1, :16], five[1])
    assert np.array_equal(kk[n - 2, :16], five[3]) and np.array_equal(kk[n - 1, :16], five[4])
    for i in range(2, n - 2):
        assert bounds[i].tolist() == [4 * i - 6, 16] and np.array_equal(kk[i, :16], five[2]), i
    # the border rows are mirror images of each other
    assert np.array_equal(five[3, :14], five[1, :14][::-1]) and np.array_equal(five[4, :10], five[0, :10][::-1])


# ------------------------------------------------------------------------------------------- C ABI, refusals, resources
def test_entries_are_declared_prototyped_and_exported_by_a_library_of_their_own():
    header = open(os.path.join(ROOT, "include", "srgd_consistency.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(srgd_[a-z0-9_]+)\s*\(", flat))
    assert declared == ENTRIES == set(CS.PROTOTYPES)
    for name, (_, argtypes) in CS.PROTOTYPES.items():
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", flat).group(1).strip()
        assert (0 if params == "void" else len(params.split(","))) == len(argtypes), name
    assert os.path.exists(CS.LIB_PATH), "build the library first (python -m srgd_amd.build)"
    assert _exports(CS.LIB_PATH) == ENTRIES
    assert CS.lib().srgd_image_consistency_last_error() is not None           # binds every prototype
    others = _exports(_lib.LIB_PATH) | _exports(MX.LIB_PATH) | _exports(EN.LIB_PATH)
    assert not ENTRIES & others and not any("consistency" in n for n in others)
    assert not any("metrics" in n or "ensemble" in n for n in ENTRIES)
    assert not set(CS.PROTOTYPES) & (set(_lib.PROTOTYPES) | set(MX.PROTOTYPES) | set(EN.PROTOTYPES))
    for phrase in ("L is the input as decoded, uint8 [h][w][3]", "O is the output AS SAVED (after --color_fix), uint8 [4h][4w][3]",
                   "D = Pillow Image.resize((w, h), BICUBIC) of O", "src/libImaging/Resample.c", "support 2.0 * 4 = 8", "a = -0.5",
                   "window clipped to the image and renormalised", "round half away from zero",
                   "horizontal pass over all 4h rows, accumulator 1 << 21, result clip8(acc >> 22), rounded to 8 bits",
                   "e = D - L", "sse_r, sse_g, sse_b = sum of e^2 per channel", "max_abs = max |e|",
                   "lr_mse = (sse_r + sse_g + sse_b) / (3*h*w)", "lr_psnr = 10*log10(255^2 / lr_mse) (+inf at 0)",
                   "32 * ceil(h / 15) * ceil(w / 32) bytes"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", header), phrase


def test_refusals_need_no_gpu():
    # every refusal is decided on the host before anything is launched, so it can be checked here: -1 and a message
    lib = CS.lib()
    off, hw = (C.c_int64 * 1)(0), (C.c_int32 * 2)(5, 5)
    p = C.c_void_p(4096)                                   # never dereferenced: a refused call launches nothing
    ok = dict(hr=p, hr_offs=off, lr=p, lr_offs=off, hw=hw, n=1, down=None, down_offs=None, stats=p, scratch=p)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.srgd_image_consistency_images(a["hr"], a["hr_offs"], a["lr"], a["lr_offs"], a["hw"], a["n"], a["down"], a["down_offs"],
                                               a["stats"], a["scratch"], None)
        return rc, lib.srgd_image_consistency_last_error().decode()
    size = lambda h, w: (C.c_int32 * 2)(h, w)              # noqa: E731
    one = lambda v: (C.c_int64 * 1)(v)                     # noqa: E731
    cases = {"null": [dict(hr=None), dict(hr_offs=None), dict(lr=None), dict(lr_offs=None), dict(hw=None), dict(stats=None),
                      dict(scratch=None)],
             "together": [dict(down=p), dict(down_offs=off)],
             "n_images": [dict(n=0), dict(n=-1)],
             "bad size": [dict(hw=size(4, 5)), dict(hw=size(5, 4)), dict(hw=size(0, 9)), dict(hw=size(9, -1))],
             "2^31 - 256": [dict(hw=size(6689, 6689)), dict(hw=size(5, 8947848))],
             "misaligned offset": [dict(hr_offs=one(8)), dict(lr_offs=one(17)), dict(down=p, down_offs=one(4))],
             "offset outside": [dict(hr_offs=one(-16)), dict(lr_offs=one(1 << 36)), dict(down=p, down_offs=one(-32))],
             "16-byte aligned": [dict(hr=C.c_void_p(4100)), dict(hr=C.c_void_p(4104))],
             "8-byte aligned": [dict(stats=C.c_void_p(4100)), dict(scratch=C.c_void_p(4100))]}
    for word, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == -1 and word in msg and msg.startswith("srgd_image_consistency_images: "), (kw, msg)
    rc = lib.srgd_image_consistency(p, p, 4, 9, None, p, p, None)
    assert rc == -1 and lib.srgd_image_consistency_last_error().decode().startswith("srgd_image_consistency: ")
    assert 48 * 5 * 8947848 == 2 ** 31 - 128 and 48 * 5 * 8947847 < 2 ** 31 - 256 <= 48 * 5 * 8947848     # the first refused width at h = 5
    assert 48 * 6689 * 6689 >= 2 ** 31 - 256 > 48 * 6688 * 6688


def test_host_side_checks_of_the_module():
    assert (CS.TILE_W, CS.TILE_H, CS.MIN_SIDE) == (K.TILE_W, K.TILE_H, 5) and CS.KEYS == K.KEYS == INF.CONSISTENCY_KEYS
    assert CS.padded(75) == 80 and CS.padded(1200) == 1200
    # the header's scratch formula: one 32-byte record per tile of 32 x 15 LR pixels
    assert CS.scratch_bytes([(5, 5)]) == 32 and CS.scratch_bytes([(15, 32)]) == 32 and CS.scratch_bytes([(16, 33)]) == 4 * 32
    assert CS.scratch_bytes([(31, 65), (5, 37)]) == 9 * 32 + 2 * 32 and CS.scratch_bytes([(320, 480)]) == 22 * 15 * 32
    with pytest.raises(ValueError, match="size"):
        CS.scratch_bytes([(4, 40)])
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)               # noqa: E731
    for outs, ins in ((u8(20, 20, 3), u8(5, 6, 3)), (u8(20, 20, 3), u8(5, 5, 4)), (u8(20, 20), u8(5, 5, 3)), (torch.zeros(20, 20, 3), u8(5, 5, 3)),
                      (u8(20, 20, 3), [u8(5, 5, 3)]), ([], []), ([u8(20, 20, 3)], [u8(5, 5, 3), u8(5, 5, 3)]), ([u8(20, 20, 3), "x"], [u8(5, 5, 3)] * 2),
                      (None, None), (u8(16, 40, 3), u8(4, 10, 3)), (u8(40, 16, 3), u8(10, 4, 3)), (u8(20, 20, 3), u8(5, 5, 3).float())):
        with pytest.raises(ValueError, match="consistency_on_device"):
            CS.consistency_on_device(outs, ins)
    with pytest.raises(_lib.SrgdHipError, match="no CPU fallback"):            # a missing GPU is an error, never another path
        CS.consistency_on_device(u8(20, 20, 3), u8(5, 5, 3))
    with pytest.raises(_lib.SrgdHipError, match="no CPU fallback"):
        CS.consistency_on_device([u8(20, 28, 3)], [u8(5, 7, 3)], return_down=True)
    for fn in ("consistency_flat", "consistency_flat_device"):
        assert list(inspect.signature(getattr(CS, fn)).parameters) == ["hr_u8", "hr_offsets", "lr_u8", "lr_offsets", "sizes", "down_u8",
                                                                        "down_offsets"]
    assert list(inspect.signature(CS.consistency_on_device).parameters) == ["outputs", "inputs", "return_down"]
    assert list(inspect.signature(CS.records).parameters) == ["stats", "sizes"]
    assert CS.records(torch.tensor([[3, 0, 0, 1], [0, 0, 0, 0]]), [(1, 1), (5, 7)]) == [K.record((3, 0, 0, 1), 1, 1), K.record((0, 0, 0, 0), 5, 7)]


def test_consistency_kernels_do_not_spill_and_fit_four_workgroups_per_cu():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_table
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "consistency.hip")) if "consistency_" in r["name"]]
    assert sorted(r["name"] for r in rows) == ["consistency_finish_kernel", "consistency_tile_kernel"]
    for r in rows:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["lds"] <= 160 * 1024 // 4 and r["vgpr"] <= 128, r       # four 256-thread workgroups per CU: LDS and registers
    assert [r["lds"] for r in rows if r["name"] == "consistency_tile_kernel"] == [72 * 448 + 72 * 96 + 320 + 64]


# ------------------------------------------------------------------------------------------- flag and document
def test_the_flag_parses_and_the_entry_is_reexported():
    assert INF.parse_args(_argv()).consistency is False
    assert INF.parse_args(_argv("--consistency")).consistency is True
    args = INF.parse_args(_argv("--consistency", "--samples", "3", "--ensemble", "--reference_dir", "gt", "--color_fix", "wavelet"))
    assert args.consistency is True and args.ensemble is True and args.samples == 3
    params = inspect.signature(INF.batch_sr_target_images).parameters
    assert params["consistency"].default is False and params["consistency_name"].default == "consistency.json"
    assert INF.consistency_on_device is CS.consistency_on_device


def test_consistency_document():
    rec = lambda a, b, c: {"lr_psnr": a, "lr_mse": b, "lr_max_abs": c}          # noqa: E731
    rows = [("a.png", "a_out.png", rec(40.0, 6.0, 9.0)), ("a.png", "a_out_s1.png", rec(42.0, 4.0, 7.0)),
            ("b.png", "b_out.png", rec(math.inf, 0.0, 0.0)), ("b.png", "b_out_s1.png", rec(30.0, 65.0, 31.0))]
    doc = json.loads(json.dumps(INF.consistency_document(rows, 2)))
    assert list(doc) == ["files", "images", "mean"]
    assert doc["files"] == {"a_out.png": rec(40.0, 6.0, 9.0), "a_out_s1.png": rec(42.0, 4.0, 7.0), "b_out.png": rec("inf", 0.0, 0.0),
                            "b_out_s1.png": rec(30.0, 65.0, 31.0)}
    assert doc["images"] == {"a.png": rec(41.0, 5.0, 8.0), "b.png": rec("inf", 32.5, 15.5)}
    assert doc["mean"] == rec("inf", 18.75, 11.75)
    single = INF.consistency_document(rows[:1], 1)
    assert list(single) == ["files", "mean"] and single["mean"] == rec(40.0, 6.0, 9.0)
    assert json.dumps(INF.consistency_document(rows, 2, ensemble=None)) == json.dumps(INF.consistency_document(rows, 2, ensemble=[]))
    full = INF.consistency_document(rows, 2, ensemble=[("a.png", rec(44.0, 2.0, 5.0)), ("b.png", rec(40.0, 6.0, 7.0))])
    assert list(full) == ["files", "images", "mean", "ensemble", "ensemble_mean"]
    assert full["ensemble"] == {"a.png": rec(44.0, 2.0, 5.0), "b.png": rec(40.0, 6.0, 7.0)} and full["ensemble_mean"] == rec(42.0, 4.0, 6.0)


# ------------------------------------------------------------------------------------------- the batch loop
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
            return ret, [{"psnr_y": 20.0, "psnr_rgb": 1.0, "ssim_y": 0.5} for _ in ims]
        return run
    monkeypatch.setattr(INF, "sr_target_image", fake("solo"))
    monkeypatch.setattr(INF, "sr_target_images", fake("same"))
    monkeypatch.setattr(INF, "sr_target_images_mixed", fake("mixed"))
    monkeypatch.setattr(INF, "sr_target_images_seeded", fake("seeded"))


def _fake_consistency(monkeypatch, batches):
    """``consistency_on_device`` replaced by the yardstick; ``batches`` records the output sizes of every batched call."""
    def run(outputs, inputs, return_down=False):
        assert isinstance(outputs, list) and isinstance(inputs, list) and len(outputs) == len(inputs) and not return_down
        assert all(t.dtype == torch.uint8 and t.dim() == 3 for t in outputs + inputs)
        batches.append([tuple(t.shape) for t in outputs])
        return [K.yardstick(o.numpy(), l.numpy())[2] for o, l in zip(outputs, inputs)]
    monkeypatch.setattr(INF, "consistency_on_device", run)


def _fake_ensemble(monkeypatch):
    def run(samples, return_mean01=False):
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


def _want(indir, outdir, written, source):
    return K.yardstick(_png(outdir / written), _png(indir / source))[2]


def test_groups_smaller_and_larger_than_k_a_small_input_and_a_run_without_samples(tmp_path, monkeypatch, capsys):
    calls, batches = [], []
    _fake_samplers(monkeypatch, calls)
    _fake_consistency(monkeypatch, batches)
    indir = _inputs(tmp_path, {"a": (64, 64), "b": (64, 64), "c": (64, 64), "d": (4, 9)})
    run = lambda tag, **kw: INF.batch_sr_target_images(str(indir), str(tmp_path / tag), None, seed=71, consistency=True, **kw)  # noqa: E731
    run("two", samples=2)                                        # groups of K: one call per flush; d is too small for the numbers
    said = capsys.readouterr().out
    assert said.count("smaller than 5 pixels on a side") == 2 and "d_out.png is 4x9" in said and "d_out_s1.png is 4x9" in said
    assert batches == [[(256, 256, 3)] * 2] * 3                    # d's flush makes no call
    names = [f"{n}_out{s}.png" for n in "abcd" for s in ("", "_s1")]
    assert sorted(os.listdir(tmp_path / "two")) == sorted(names + ["consistency.json"])
    doc = json.load(open(tmp_path / "two" / "consistency.json"))
    assert list(doc) == ["files", "images", "mean"] and list(doc["files"]) == names[:6] and list(doc["images"]) == ["a.png", "b.png", "c.png"]
    for n in "abc":
        recs = [_want(indir, tmp_path / "two", f"{n}_out{s}.png", f"{n}.png") for s in ("", "_s1")]
        assert [doc["files"][f"{n}_out{s}.png"] for s in ("", "_s1")] == recs
        assert doc["images"][f"{n}.png"] == {k: (recs[0][k] + recs[1][k]) / 2 for k in K.KEYS}
    assert doc["mean"] == {k: sum(doc["images"][f"{n}.png"][k] for n in "abc") / 3 for k in K.KEYS}
    batches.clear()
    run("three", samples=2, lockstep=3)                          # a a b | b c c | d d: groups larger than K
    assert batches == [[(256, 256, 3)] * 3] * 2
    assert json.load(open(tmp_path / "three" / "consistency.json")) == doc
    batches.clear()
    run("one", samples=2, lockstep_tiles=1, end_index=3)         # every sample alone: groups smaller than K (d cannot be tiled)
    assert batches == [[(256, 256, 3)]] * 6 and [c[0] for c in calls[-6:]] == ["solo"] * 6
    assert json.load(open(tmp_path / "one" / "consistency.json")) == doc
    batches.clear()
    run("plain")                                                 # no --samples: no "images"
    plain = json.load(open(tmp_path / "plain" / "consistency.json"))
    assert list(plain) == ["files", "mean"] and list(plain["files"]) == ["a_out.png", "b_out.png", "c_out.png"]
    assert plain["files"] == {k: v for k, v in doc["files"].items() if k in plain["files"]}
    # a second run over complete outputs samples nothing: no call, the file stays as it is
    before = open(tmp_path / "plain" / "consistency.json").read()
    batches.clear()
    run("plain")
    assert batches == [] and open(tmp_path / "plain" / "consistency.json").read() == before
    run("ranked", consistency_name="consistency_rank3.json")
    assert "consistency_rank3.json" in os.listdir(tmp_path / "ranked") and "consistency.json" not in os.listdir(tmp_path / "ranked")


def test_the_ensemble_entry_and_runs_without_the_flag(tmp_path, monkeypatch):
    calls, batches = [], []
    _fake_samplers(monkeypatch, calls)
    _fake_consistency(monkeypatch, batches)
    _fake_ensemble(monkeypatch)
    monkeypatch.setattr(INF, "metrics_on_device", lambda outs, refs, crop_border=4: [{"psnr_y": 30.0, "psnr_rgb": 2.0, "ssim_y": 0.25} for _ in refs])
    indir, gt = _inputs(tmp_path, {"a": (64, 64), "b": (64, 64)}), tmp_path / "gt"
    gt.mkdir()
    for name in "ab":
        Image.fromarray(np.full((256, 256, 3), 10, dtype=np.uint8), "RGB").save(gt / f"{name}.png")
    run = lambda tag, **kw: INF.batch_sr_target_images(str(indir), str(tmp_path / tag), None, seed=71, samples=2, **kw)  # noqa: E731
    run("ens", ensemble=True, consistency=True)
    # per flush: the group's samples, then the mean image of the file it completed
    assert batches == [[(256, 256, 3)] * 2, [(256, 256, 3)]] * 2
    doc = json.load(open(tmp_path / "ens" / "consistency.json"))
    assert list(doc) == ["files", "images", "mean", "ensemble", "ensemble_mean"] and list(doc["ensemble"]) == ["a.png", "b.png"]
    for n in "ab":
        assert doc["ensemble"][f"{n}.png"] == _want(indir, tmp_path / "ens", f"{n}_out_mean.png", f"{n}.png")
        assert doc["files"][f"{n}_out_s1.png"] == _want(indir, tmp_path / "ens", f"{n}_out_s1.png", f"{n}.png")
    assert doc["ensemble_mean"] == {k: (doc["ensemble"]["a.png"][k] + doc["ensemble"]["b.png"][k]) / 2 for k in K.KEYS}
    # the mean of K random samples is closer to nothing in particular, but it is an image of its own: not one of the files' records
    assert doc["ensemble"]["a.png"] != doc["files"]["a_out.png"]
    # without --consistency: no call, no file; metrics.json and ensemble.json byte for byte what the flagged run writes beside it
    batches.clear()
    run("both", ensemble=True, reference_dir=str(gt), consistency=True)
    run("neither", ensemble=True, reference_dir=str(gt))
    assert batches == [[(256, 256, 3)] * 2, [(256, 256, 3)]] * 2                 # all from "both"
    assert sorted(os.listdir(tmp_path / "neither")) == sorted(set(os.listdir(tmp_path / "both")) - {"consistency.json"})
    assert sorted(os.listdir(tmp_path / "neither")) == sorted([f"{n}_out{s}.png" for n in "ab" for s in ("", "_s1", "_mean", "_std")]
                                                              + ["ensemble.json", "metrics.json"])
    for n in os.listdir(tmp_path / "neither"):
        assert open(tmp_path / "neither" / n, "rb").read() == open(tmp_path / "both" / n, "rb").read(), n
    assert json.load(open(tmp_path / "both" / "consistency.json")) == doc
    # --reference_dir alone: the files written are the ones written today
    run("ref", reference_dir=str(gt))
    assert sorted(os.listdir(tmp_path / "ref")) == sorted([f"{n}_out{s}.png" for n in "ab" for s in ("", "_s1")] + ["metrics.json"])
    assert list(json.load(open(tmp_path / "ref" / "metrics.json"))) == ["crop_border", "files", "images", "mean"]
