"""``--reference_dir``: Y-channel PSNR, RGB PSNR and Y-channel SSIM of the sampler's output against its ground truth, on the GPU
(srgd_image_metrics / srgd_image_metrics_images of libsrgd_metrics.so, srgd_amd/csrc/metrics.hip).

Yardstick: tests/metrics_cases.py - the definition of include/srgd_metrics.h restated literally in float64 numpy, the 2-D 121-tap
window as a double loop.  Gates (derived there from the number formats, not from what the kernels give): |ssim - ssim_ref| <= 1e-9,
|psnr - psnr_ref| <= 1e-9 dB for finite values, inf and NaN by kind.  Everything else here is exact: the four doubles of an image
bitwise equal alone and in any group, bytes of srgd_image_unit_to_u8 equal to the restatement's quantisation, PNG files byte for
byte with and without --reference_dir."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import _lib
from srgd_amd import inference as INF
from srgd_amd import metrics as MX
from srgd_amd.synth import synth_state_dict
from tests import metrics_cases as M
from tests.test_engine_gpu import _schema, build_edm_sampler, build_sampler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0
GROUP = [(19, 19), (23, 27), (300, 500)]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _solo(out01, ref, crop):
    """srgd_image_metrics on one ([3,h,w] float32, [h,w,3] uint8) numpy pair: the four doubles as a CPU tensor."""
    h, w = out01.shape[1:]
    o, r = torch.from_numpy(np.ascontiguousarray(out01)).cuda(), torch.from_numpy(np.ascontiguousarray(ref)).cuda()
    res = torch.full((4,), SENTINEL, device="cuda", dtype=torch.float64)
    scratch = torch.empty(MX.scratch_doubles([(h, w)], crop), device="cuda", dtype=torch.float64)
    rc = MX.lib().srgd_image_metrics(_p(o), _p(r), h, w, crop, _p(res), _p(scratch), _stream())
    assert rc == 0, MX.lib().srgd_image_metrics_last_error()
    torch.cuda.synchronize()
    return res.cpu()


def _group(pairs, crop, out_gap=3, ref_gap=5, lead=1):
    """srgd_image_metrics_images on pairs packed into flat buffers at offsets that are no multiples of 4: [n,4] CPU tensor."""
    sizes = [p[0].shape[1:] for p in pairs]
    o_offs, r_offs, o_end, r_end = [], [], lead, lead
    for (h, w) in sizes:
        o_offs.append(o_end)
        r_offs.append(r_end)
        o_end += 3 * h * w + out_gap
        r_end += 3 * h * w + ref_gap
    assert any(o % 4 for o in o_offs) and any(r % 4 for r in r_offs)
    out = torch.full((o_end,), 0.5, dtype=torch.float32)
    ref = torch.zeros(r_end, dtype=torch.uint8)
    for (o01, r8), oo, ro in zip(pairs, o_offs, r_offs):
        out[oo:oo + o01.size] = torch.from_numpy(np.ascontiguousarray(o01)).reshape(-1)
        ref[ro:ro + r8.size] = torch.from_numpy(np.ascontiguousarray(r8)).reshape(-1)
    return MX.metrics_flat_device(out.cuda(), ref.cuda(), o_offs, r_offs, sizes, crop).cpu()


def _bits(t):
    return t.contiguous().view(torch.int64)


def _check(got4, want, what):
    for k, key in enumerate(M.KEYS):
        g = float(got4[k])
        print(f"{what} {key}: gpu {g!r} restatement {want[key]!r} diff {abs(g - want[key]) if math.isfinite(g) and math.isfinite(want[key]) else 'kind'}")
        assert M.same_kind_or_close(g, want[key]), (what, key, g, want[key])


# ------------------------------------------------------------------------------------------- 1. against the restatement
def _cases(crop):
    shapes = [(19, 19), (23, 27)] + M.edge_shapes(crop) + [(300, 500)]
    cases = [M.case("random", h, w, crop, 100 + i) for i, (h, w) in enumerate(shapes)]
    return cases + [M.case("noisy", 64, 80, crop, 7), M.case("noisy", 27, 75, crop, 8)]


@pytest.mark.parametrize("crop", [0, 4])
def test_both_entries_against_the_float64_restatement(crop):
    cases = _cases(crop)
    for out01, ref, want in cases:
        got = _solo(out01, ref, crop)
        _check(got, want, f"C ABI {out01.shape[1:]} crop {crop}")
        assert float(got[3]) == 0.0
    # the Python entry, every case in one batched call (list form), and the tensor form on one of them
    recs = MX.metrics_on_device([torch.from_numpy(o)[None].cuda() for o, _, _ in cases], [torch.from_numpy(r) for _, r, _ in cases], crop)
    assert len(recs) == len(cases) and all(set(r) == set(M.KEYS) and all(type(v) is float for v in r.values()) for r in recs)
    for rec, (out01, ref, want) in zip(recs, cases):
        _check([rec[k] for k in M.KEYS], want, f"metrics_on_device {out01.shape[1:]} crop {crop}")
    out01, ref, want = cases[1]
    for o, r in ((torch.from_numpy(out01).cuda(), torch.from_numpy(ref)), (torch.from_numpy(out01)[None].cuda(), torch.from_numpy(ref)[None].cuda())):
        (rec,) = MX.metrics_on_device(o, r, crop)
        assert rec == recs[1]
    two = MX.metrics_on_device(torch.from_numpy(np.stack([out01, out01])).cuda(), [torch.from_numpy(ref)] * 2, crop)
    assert two == [recs[1], recs[1]]


def test_identical_images_and_a_crop_that_removes_the_difference_give_inf():
    out01, _ = M.pair(24, 30, 3)
    ref = M.quantise(out01).astype(np.uint8)
    got = _solo(out01, ref, 0)
    assert float(got[0]) == math.inf and float(got[1]) == math.inf and abs(float(got[2]) - 1.0) <= 1e-12
    ref[0, 5] ^= 255
    ref[20, 29] ^= 255
    ref[3, 3] ^= 255
    _check(_solo(out01, ref, 0), M.restate(out01, ref, 0), "three differing pixels, crop 0")
    cut = _solo(out01, ref, 4)
    assert float(cut[0]) == math.inf and float(cut[1]) == math.inf and abs(float(cut[2]) - 1.0) <= 1e-12


# ------------------------------------------------------------------------------------------- 2. quantisation
def test_quantisation_is_unit_to_u8s_product_and_truncation():
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    vals = np.concatenate([k, np.nextafter(k, np.float32(2.0)), np.nextafter(k, np.float32(-1.0))])
    vals = np.clip(vals, 0.0, 1.0).astype(np.float32)             # 768 values: k/255 and its two neighbours, inside [0,1]
    h, w = 24, 32
    out01 = np.stack([np.roll(vals, 97 * c).reshape(h, w) for c in range(3)])
    ref = M.pair(h, w, 11)[1]
    for crop in (0, 4):
        _check(_solo(out01, ref, crop), M.restate(out01, ref, crop), f"k/255 neighbours crop {crop}")
    # against the quantised image itself as reference a single wrong level would show as a finite PSNR
    q = M.quantise(out01)
    got = _solo(out01, q.astype(np.uint8), 0)
    assert float(got[0]) == math.inf and float(got[1]) == math.inf
    u8 = INF.unit_tensor_to_u8_on_device(torch.from_numpy(out01).cuda()).cpu().numpy()
    assert u8.dtype == np.uint8 and np.array_equal(u8.astype(np.int64), q)


# ------------------------------------------------------------------------------------------- 3. / 4. bit-identity
def test_an_image_is_bitwise_itself_in_any_group_and_at_any_offset():
    pairs = [M.pair(h, w, 40 + i) for i, (h, w) in enumerate(GROUP)]
    for crop in (0, 4):
        solos = [_solo(o, r, crop) for o, r in pairs]
        for order in ((0, 1, 2), (2, 0, 1)):
            got = _group([pairs[i] for i in order], crop)
            for row, i in zip(got, order):
                assert torch.equal(_bits(row), _bits(solos[i])), (crop, order, i, row, solos[i])
        shifted = _group(pairs, crop, out_gap=6, ref_gap=1, lead=2)
        assert all(torch.equal(_bits(row), _bits(s)) for row, s in zip(shifted, solos))


def test_more_than_128_images_in_one_call():
    out01, ref = M.pair(19, 19, 40)
    other = M.pair(23, 27, 41)
    solo, solo_other = _solo(out01, ref, 4), _solo(*other, 4)
    pairs = [(out01, ref)] * 130
    pairs[128] = other                                            # the second launch sequence is not a copy of the first
    got = _group(pairs, 4)
    assert got.shape == (130, 4)
    for i, row in enumerate(got):
        assert torch.equal(_bits(row), _bits(solo_other if i == 128 else solo)), i


# ------------------------------------------------------------------------------------------- 5. non-finite values
def test_a_non_finite_value_is_nan_for_its_image_alone_and_only_inside_the_crop():
    pairs = [M.pair(h, w, 40 + i) for i, (h, w) in enumerate(GROUP)]
    clean = _group(pairs, 4)
    assert bool(torch.isfinite(clean).all())
    for value in (np.nan, np.inf):
        bad = pairs[1][0].copy()
        bad[2, 10, 12] = value
        got = _group([pairs[0], (bad, pairs[1][1]), pairs[2]], 4)
        assert bool(torch.isnan(got[1, :3]).all()) and float(got[1, 3]) == 1.0, got[1]
        assert torch.equal(_bits(got[0]), _bits(clean[0])) and torch.equal(_bits(got[2]), _bits(clean[2]))
        assert all(math.isnan(v) for v in M.restate(bad, pairs[1][1], 4).values())
    bad = pairs[1][0].copy()
    bad[0, 4, 4] = -np.inf                                        # first pixel inside the crop, and two values of one pixel
    bad[1, 4, 4] = np.nan
    got = _group([pairs[0], (bad, pairs[1][1]), pairs[2]], 4)
    assert bool(torch.isnan(got[1, :3]).all()) and float(got[1, 3]) == 2.0
    for (y, x) in ((2, 12), (3, 3), (10, 23), (19, 0)):           # the 4-pixel border of the 23x27 image: never read
        edge = pairs[1][0].copy()
        edge[2, y, x] = np.nan
        got = _group([pairs[0], (edge, pairs[1][1]), pairs[2]], 4)
        assert torch.equal(_bits(got), _bits(clean)), (y, x)
    recs = MX.metrics_on_device([torch.from_numpy(bad)[None].cuda()], [torch.from_numpy(pairs[1][1])], 4)
    assert all(math.isnan(v) for v in recs[0].values())


# ------------------------------------------------------------------------------------------- 6. errors
def test_refusals_write_nothing_and_leave_the_library_usable():
    lib = MX.lib()
    fn = lib.srgd_image_metrics_images
    out = torch.rand(3 * 18 * 40 + 3 * 30 * 30, device="cuda")
    ref = torch.zeros(out.numel(), dtype=torch.uint8, device="cuda")
    res = torch.full((2, 4), SENTINEL, device="cuda", dtype=torch.float64)
    scratch = torch.full((64,), SENTINEL, device="cuda", dtype=torch.float64)
    i64, i32 = lambda *v: (C.c_int64 * len(v))(*v), lambda *v: (C.c_int32 * len(v))(*v)         # noqa: E731

    def untouched():
        torch.cuda.synchronize()
        return bool((res == SENTINEL).all()) and bool((scratch == SENTINEL).all())
    # an 18x40 image at crop 4 keeps 10 rows: no SSIM position
    rc = lib.srgd_image_metrics(_p(out), _p(ref), 18, 40, 4, _p(res), _p(scratch), _stream())
    assert rc < 0 and b"11 x 11" in lib.srgd_image_metrics_last_error() and untouched()
    assert lib.srgd_image_metrics(_p(out), _p(ref), 40, 18, 4, _p(res), _p(scratch), _stream()) < 0 and untouched()
    # ... also as the SECOND image of a group: every image is checked before the first launch
    offs = i64(3 * 18 * 40, 0)
    assert fn(_p(out), _p(ref), offs, offs, i32(30, 30, 18, 40), 2, 4, _p(res), _p(scratch), _stream()) < 0 and untouched()
    assert fn(_p(out), _p(ref), offs, offs, i32(30, 30, 18, 40), 2, -1, _p(res), _p(scratch), _stream()) < 0 and untouched()
    assert fn(_p(out), _p(ref), i64(-1), i64(0), i32(30, 30), 1, 4, _p(res), _p(scratch), _stream()) < 0 and untouched()
    assert fn(_p(out), None, i64(0), i64(0), i32(30, 30), 1, 4, _p(res), _p(scratch), _stream()) < 0 and untouched()
    assert fn(_p(out), _p(ref), i64(0), i64(0), i32(30, 30), -1, 4, _p(res), _p(scratch), _stream()) < 0 and untouched()
    # no image: nothing to do, and that is not an error
    assert fn(_p(out), _p(ref), i64(0), i64(0), i32(30, 30), 0, 4, _p(res), _p(scratch), _stream()) == 0 and untouched()
    assert MX.metrics_flat(out, ref, [], [], [], 4) == []
    with pytest.raises(ValueError, match="11x11"):
        MX.metrics_on_device(torch.rand(3, 18, 40).cuda(), torch.zeros(18, 40, 3, dtype=torch.uint8), 4)
    with pytest.raises(ValueError, match="do not fit"):
        MX.metrics_flat(out, ref, [out.numel() - 10], [0], [(30, 30)], 4)
    with pytest.raises(_lib.SrgdHipError, match="no CPU fallback"):
        MX.metrics_on_device(torch.rand(3, 30, 30), torch.zeros(30, 30, 3, dtype=torch.uint8), 4)
    # the same 18x40 image at crop 3 is fine, and so is the library
    o18, r18 = M.pair(18, 40, 5)
    _check(_solo(o18, r18, 3), M.restate(o18, r18, 3), "18x40 crop 3")


# ------------------------------------------------------------------------------------------- 7. end to end
def _run(sampler, seed, **kw):
    torch.manual_seed(seed)
    sampler.device_noise_seed = seed
    return sampler.tiled_sample(**kw)


def test_tiled_sample_reference_keyword():
    sampler = build_sampler(16)
    g = torch.Generator().manual_seed(21)
    sizes = [(256, 256), (300, 260)]
    conds = [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in sizes]
    refs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for (h, w) in sizes]
    kw = dict(batch_size=8, num_sample_steps=2, precision="bf16", class_label=torch.tensor([1]).cuda())
    plain = _run(sampler, 5, condition_x=conds, color_fix="wavelet", **kw)
    assert isinstance(plain, list) and torch.is_tensor(plain[0])                  # without the keyword: the return value as it was
    outs, quality = _run(sampler, 5, condition_x=conds, color_fix="wavelet", reference=refs, **kw)
    assert all(torch.equal(a, b) for a, b in zip(outs, plain))
    assert quality == MX.metrics_on_device(plain, refs) and len(quality) == 2       # after the colour fix, default crop 4
    raw = _run(sampler, 5, condition_x=conds, **kw)
    assert quality != MX.metrics_on_device(raw, refs)
    q0 = M.restate(plain[0][0].cpu().numpy(), refs[0].numpy(), 4)
    _check([quality[0][k] for k in M.KEYS], q0, "tiled_sample 256x256")
    # seeds: K samples of one image against the same reference; crop_border is handed on
    outs2, quality2 = _run(sampler, 9, condition_x=[conds[1], conds[1]], seeds=[5, 6], color_fix="wavelet",
                           reference=[refs[1], refs[1]], crop_border=0, **kw)
    assert torch.equal(outs2[0], plain[1]) and quality2 == MX.metrics_on_device(outs2, [refs[1]] * 2, 0)
    assert quality2[0] != quality2[1] and quality2[0] != quality[1]
    # the [B,3,H,W] form, alone and with trajectories, and the EDM wrapper
    batch, bref = conds[0], refs[0]
    out, qb = _run(sampler, 5, condition_x=batch, reference=bref, **kw)
    assert torch.equal(out, _run(sampler, 5, condition_x=batch, **kw)) and qb == MX.metrics_on_device(out, bref)
    ret = _run(sampler, 5, condition_x=batch, reference=[bref], with_images=True, with_x0_images=True, **kw)
    assert len(ret) == 4 and torch.equal(ret[0], out) and ret[3] == qb
    edm = build_edm_sampler(16)
    ekw = dict(batch_size=8, num_sample_steps=2, precision="bf16", class_label=torch.tensor([0]).cuda())
    eout, eq = _run(edm, 6, condition_x=batch, reference=bref, **ekw)
    assert torch.equal(eout, _run(edm, 6, condition_x=batch, **ekw)) and eq == MX.metrics_on_device(eout, bref)
    # refusals, before any sampling: a wrong reference, an image too small for the crop, a sharded canvas
    with pytest.raises(ValueError, match="references for"):
        sampler.tiled_sample(condition_x=conds, reference=refs[:1], **kw)
    with pytest.raises(ValueError, match="uint8"):
        sampler.tiled_sample(condition_x=conds, reference=[refs[1], refs[0]], **kw)
    with pytest.raises(ValueError, match="11x11"):
        sampler.tiled_sample(condition_x=conds, reference=refs, crop_border=123, **kw)
    sampler.canvas_group = object()
    try:
        with pytest.raises(NotImplementedError, match="canvas_group"):
            sampler.tiled_sample(condition_x=batch, reference=bref, **kw)
    finally:
        sampler.canvas_group = None


def test_cli_reference_dir_writes_metrics_json(tmp_path):
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    indir, gt = tmp_path / "in", tmp_path / "gt"
    indir.mkdir()
    gt.mkdir()
    rng = np.random.default_rng(4)
    for name, (h, w) in (("a", (40, 56)), ("b", (64, 48))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(indir / f"{name}.png")
        Image.fromarray(rng.integers(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8), "RGB").save(gt / f"{name}.png")
    argv = ["-c", str(conf), "-m", str(ckpt), "--input_dir", str(indir), "--num_sample_steps", "2", "--test_label", "1",
            "--batch_size", "4", "--device_noise", "--seed", "71", "--precision", "bf16", "--color_fix", "wavelet",
            "--lockstep_tiles", "16", "--samples", "2"]
    out_m, out_p = tmp_path / "out_metrics", tmp_path / "out_plain"
    INF.main(argv + ["--output_dir", str(out_m), "--reference_dir", str(gt)])
    INF.main(argv + ["--output_dir", str(out_p)])
    written = ["a_out.png", "a_out_s1.png", "b_out.png", "b_out_s1.png"]
    assert sorted(p.name for p in out_p.iterdir()) == written                       # no metrics.json without the flag
    assert sorted(p.name for p in out_m.iterdir()) == written + ["metrics.json"]
    for name in written:
        assert (out_m / name).read_bytes() == (out_p / name).read_bytes(), name     # the numbers change no output
    doc = json.load(open(out_m / "metrics.json"))
    assert doc["crop_border"] == 4 and list(doc["files"]) == written and list(doc["images"]) == ["a.png", "b.png"]
    assert doc["files"]["a_out.png"] != doc["files"]["a_out_s1.png"]                # two samples of one image
    for name in written:
        png = np.asarray(Image.open(out_m / name).convert("RGB"))
        ref = np.asarray(Image.open(gt / (name[0] + ".png")).convert("RGB"))
        _check([doc["files"][name][k] for k in M.KEYS], M.restate_u8(png, ref, 4), f"metrics.json {name}")
    mean = lambda recs: {k: sum(r[k] for r in recs) / len(recs) for k in M.KEYS}    # noqa: E731
    for n in "ab":
        assert doc["images"][f"{n}.png"] == mean([doc["files"][f"{n}_out.png"], doc["files"][f"{n}_out_s1.png"]])
    assert doc["mean"] == mean([doc["images"]["a.png"], doc["images"]["b.png"]])
    # a missing reference ends the run before anything is sampled or written
    os.remove(gt / "b.png")
    out_x = tmp_path / "out_missing"
    with pytest.raises(SystemExit, match="b.png"):
        INF.main(argv + ["--output_dir", str(out_x), "--reference_dir", str(gt)])
    assert not out_x.exists()
