"""Iterative back-projection on the GPU (srgd_amd/csrc/backproject.hip, include/srgd_backproject.h) against Pillow itself
(tests/backproject_cases.py).  Everything between the two quantisations is 8-bit and the result is ``u8 / 255``: every comparison here
is an equality.
LR sizes (h x w; a tile is 15 rows x 32 columns of LR pixels = 60 x 128 HR pixels): 5x5 (every index a border index or of the single
interior phase run), 5x37, 37x5 and 6x7 (odd w: the HR rows are not 16-byte aligned), 8x8 (aligned), 16x33 (a full tile and a 1-pixel
remainder tile on each axis), 31x65 (two full tiles and a 1-pixel remainder both ways).  tests/test_backproject_cpu.py shows that on
every one of these inputs the clip acts both ways and LR-MSE falls in each of five iterations."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import backproject as BP
from srgd_amd import inference as INF
from srgd_amd import metrics as MX
from tests import backproject_cases as B
from tests import consistency_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY_F = -7.25                                             # beyond dst01 and in the gaps of the flat buffers
CANARY_B = 0xA5                                              # beyond the scratch
TAIL = 64


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _flat(a):
    return torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)


def _call_images(items, gaps, n, in_place=False):
    """``srgd_image_backproject_images`` on ``items`` = [(out01 [3,H,W], cond01 [3,H,W])] laid out in order with ``gaps[j]`` canary
    elements in front of image j in all three buffers, the scratch canary-filled beyond its size.  -> per image dst01 [3,H,W] numpy;
    asserts that every canary - gaps, tails, beyond the scratch - is untouched and that out01 / cond01 are left as they were."""
    sizes = [(o.shape[1] // 4, o.shape[2] // 4) for o, _ in items]
    offs, total = [], 0
    for (o, _), gap in zip(items, gaps):
        total += gap
        offs.append(total)
        total += o.size
    host_out = torch.full((total + TAIL,), CANARY_F, dtype=torch.float32)
    host_cond = host_out.clone()
    used = torch.zeros(total + TAIL, dtype=torch.bool)
    for (o, c), off in zip(items, offs):
        host_out[off:off + o.size] = _flat(o)
        host_cond[off:off + c.size] = _flat(c)
        used[off:off + o.size] = True
    out, cond = host_out.cuda(), host_cond.cuda()
    dst = out if in_place else torch.full((total + TAIL,), CANARY_F, dtype=torch.float32, device="cuda")
    nbytes = BP.scratch_bytes(sizes)
    scratch = torch.full((nbytes + 256,), CANARY_B, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 256 == 0
    k = len(items)
    rc = BP.lib().srgd_image_backproject_images(_p(out), _p(cond), (C.c_int64 * k)(*offs), (C.c_int32 * (2 * k))(*[v for s in sizes for v in s]),
                                                k, n, _p(dst), _p(scratch), _stream())
    assert rc == 0, BP.lib().srgd_image_backproject_last_error()
    torch.cuda.synchronize()
    got = dst.cpu()
    assert (scratch[nbytes:] == CANARY_B).all()
    assert (got[~used] == CANARY_F).all()                        # gaps and the tail of dst01 (of out01, in place) come back untouched
    same = lambda a, b: np.array_equal(a.numpy(), b.numpy(), equal_nan=True)           # noqa: E731
    assert same(cond.cpu(), host_cond) and (in_place or same(out.cpu(), host_out))
    return [got[off:off + o.size].view(o.shape).numpy() for (o, _), off in zip(items, offs)]


def _call_single(out01, cond01, n):
    """``srgd_image_backproject`` on one image, canaries beyond dst01 and the scratch -> dst01 [3,H,W] numpy."""
    h, w = out01.shape[1] // 4, out01.shape[2] // 4
    out, cond = _flat(out01).cuda(), _flat(cond01).cuda()
    dst = torch.full((out01.size + TAIL,), CANARY_F, dtype=torch.float32, device="cuda")
    nbytes = BP.scratch_bytes([(h, w)])
    scratch = torch.full((nbytes + 256,), CANARY_B, dtype=torch.uint8, device="cuda")
    rc = BP.lib().srgd_image_backproject(_p(out), _p(cond), h, w, n, _p(dst), _p(scratch), _stream())
    assert rc == 0, BP.lib().srgd_image_backproject_last_error()
    torch.cuda.synchronize()
    assert (scratch[nbytes:] == CANARY_B).all() and (dst[out01.size:] == CANARY_F).all()
    same = lambda t, a: np.array_equal(t.cpu().numpy(), np.ravel(a), equal_nan=True)   # noqa: E731
    assert same(out, out01) and same(cond, cond01)               # out of place: the inputs are left as they were
    return dst[:out01.size].view(out01.shape).cpu().numpy()


def _check(got, want_u8, what):
    """Both forms of the comparison: dst01 == yard / 255 in float32, and q(dst01) == yard."""
    print(f"{what}: differs from the yardstick in {int((B.quant_out(got).transpose(1, 2, 0) != want_u8).sum())} of {want_u8.size} bytes")
    assert got.dtype == np.float32 and np.array_equal(got, B.unit(want_u8)), what
    assert np.array_equal(B.quant_out(got).transpose(1, 2, 0), want_u8), what


# ------------------------------------------------------------------------------------------- 1. both entries against Pillow
@pytest.mark.parametrize("h,w", B.SIZES)
def test_both_entries_equal_the_yardstick(h, w):
    cases = [B.case(kind, h, w) for kind in B.KINDS]
    for n in (1, 2, 5):
        for kind, (out, cond, _, seq) in zip(B.KINDS, cases):
            _check(_call_single(B.unit(out), B.unit(cond), n), seq[n], f"single {kind} {h}x{w} N={n}")
        got = _call_images([(B.unit(out), B.unit(cond)) for out, cond, _, _ in cases], [0, 0, 0], n)       # ONE batched call
        for kind, (_, _, _, seq), g in zip(B.KINDS, cases, got):
            _check(g, seq[n], f"images {kind} {h}x{w} N={n}")
    # the Python layer: a list, a batch tensor and a single [3,H,W] tensor
    outs = [torch.from_numpy(B.unit(c[0]))[None].cuda() for c in cases]
    conds = [torch.from_numpy(B.unit(c[1]))[None].cuda() for c in cases]
    kept = [o.clone() for o in outs]
    res = BP.back_project_on_device(outs, conds, 2)
    assert all(torch.equal(a, b) for a, b in zip(outs, kept))        # out is left as it is
    for c, r in zip(cases, res):
        assert r.shape == (1, 3, 4 * h, 4 * w) and np.array_equal(r[0].cpu().numpy(), B.unit(c[3][2]))
    batch = BP.back_project_on_device(torch.cat(outs, 0), torch.cat(conds, 0), 2)
    assert batch.shape == (3, 3, 4 * h, 4 * w) and all(torch.equal(batch[i:i + 1], res[i]) for i in range(3))
    assert torch.equal(BP.back_project_on_device(outs[1][0], conds[1][0], 2), res[1][0])


def test_constant_images():
    for a, b in ((0, 255), (255, 0), (17, 200), (77, 77)):
        got = _call_single(B.unit(K.constant(32, 28, a)), B.unit(K.constant(32, 28, b)), 2)
        assert np.array_equal(got, B.unit(K.constant(32, 28, b))), (a, b)


# ------------------------------------------------------------------------------------------- 2. in place; alone, in a group, anywhere
def test_in_place_equals_out_of_place():
    items = [(B.unit(B.case(kind, h, w)[0]), B.unit(B.case(kind, h, w)[1])) for kind, (h, w) in (("random", (16, 33)), ("overshoot", (6, 7)),
                                                                                                    ("up", (5, 37)))]
    apart = _call_images(items, [0, 8, 3], 3)                        # asserts that out01 and cond01 are untouched
    inside = _call_images(items, [0, 8, 3], 3, in_place=True)
    for a, b in zip(apart, inside):
        assert np.array_equal(a, b)
    _check(inside[0], B.case("random", 16, 33)[3][3], "in place 16x33")
    out = torch.from_numpy(items[0][0]).reshape(-1).cuda()
    cond = torch.from_numpy(items[0][1]).reshape(-1).cuda()
    assert BP.back_project_flat(out, cond, [0], [(64, 132)], 3) is out         # the Python layer: dst=None is in place
    assert np.array_equal(out.view(3, 64, 132).cpu().numpy(), apart[0])


def test_an_image_is_bit_identical_alone_in_a_group_and_at_any_offset():
    shapes = [(5, 5), (5, 37), (6, 7), (8, 8), (16, 33), (31, 65)]
    items = [(B.unit(B.case("random", h, w)[0]), B.unit(B.case("random", h, w)[1])) for (h, w) in shapes]
    alone = [_call_single(o, c, 2) for o, c in items]
    for (h, w), got in zip(shapes, alone):
        _check(got, B.case("random", h, w)[3][2], f"alone {h}x{w}")
    order = [3, 5, 0, 2, 4, 1]
    # offsets that are multiples of 4 elements (16-byte accesses) and offsets that are not (4-byte accesses)
    layouts = [(list(range(6)), _call_images(items, [0] * 6, 2)),
               (order, _call_images([items[i] for i in order], [4, 12, 1024, 0, 4096, 40], 2)),
               (order[::-1], _call_images([items[i] for i in order[::-1]], [1, 2, 0, 7, 1029, 3], 2)),
               (order, _call_images([items[i] for i in order], [3, 5, 0, 2, 1, 9], 2, in_place=True))]
    for idx, got in layouts:
        for pos, i in enumerate(idx):
            assert np.array_equal(got[pos], alone[i]), (idx, i)
    twice = _call_images([items[4], items[1], items[4]], [32, 0, 81], 2)         # the same image twice in one call
    assert np.array_equal(twice[0], alone[4]) and np.array_equal(twice[2], alone[4]) and np.array_equal(twice[1], alone[1])


def test_more_than_128_images_in_one_call():
    n = 130
    pairs = [K.random_pair(5, 5, 700 + i) for i in range(n)]
    conds = [K.pillow_up(lr) for _, lr in pairs]
    res = BP.back_project_on_device([torch.from_numpy(B.unit(o))[None].cuda() for o, _ in pairs],
                                    [torch.from_numpy(B.unit(c))[None].cuda() for c in conds], 2)
    assert len(res) == n
    for i, ((out, _), cond, r) in enumerate(zip(pairs, conds, res)):
        assert np.array_equal(r[0].cpu().numpy(), B.unit(B.steps(out, cond, 2)[2])), i


# ------------------------------------------------------------------------------------------- 3. non-finite values, saturation
def test_non_finite_values_stay_visible_and_values_outside_the_unit_interval_saturate():
    out, cond, _, _ = B.case("random", 16, 33)
    out01, cond01 = B.unit(out).copy(), B.unit(cond).copy()
    planted = {(0, 0, 0): np.nan, (1, 63, 131): np.inf, (2, 30, 64): -np.inf, (0, 59, 127): np.nan, (1, 60, 128): np.inf,
               (2, 0, 131): -np.inf, (0, 17, 5): np.inf}
    for at, v in planted.items():
        out01[at] = v
    out01[1, 5, 5], out01[2, 40, 100], out01[0, 63, 0] = -0.3, 1.7, 1.7          # finite, outside [0,1]: they saturate
    cond01[0, 3, 3], cond01[2, 63, 131] = np.nan, np.nan                         # NaN in the condition counts as 0
    start, c_u8 = B.quant_out(out01).transpose(1, 2, 0), B.quant_cond(cond01).transpose(1, 2, 0)
    assert start[0, 0, 0] == 0 and start[63, 131, 1] == 255 and start[30, 64, 2] == 0
    assert start[5, 5, 1] == 0 and start[40, 100, 2] == 255 and start[63, 0, 0] == 255
    assert c_u8[3, 3, 0] == 0 and c_u8[63, 131, 2] == 0
    for n in (1, 3):
        want = B.unit(B.steps(np.ascontiguousarray(start), np.ascontiguousarray(c_u8), n)[n])
        for at, v in planted.items():
            want[at] = v
        for got in (_call_single(out01, cond01, n), _call_images([(out01, cond01)], [5], n)[0], _call_images([(out01, cond01)], [8], n, in_place=True)[0]):
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got, want, equal_nan=True), n
            assert np.isfinite(got).sum() == got.size - len(planted)


# ------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_write_nothing_and_leave_the_library_usable():
    lib = BP.lib()
    out_u8, cond_u8, _, seq = B.case("random", 6, 7)
    e = out_u8.size
    bufs = dict(out=torch.cat([_flat(B.unit(out_u8)), torch.full((e,), CANARY_F)]).cuda(),
                cond=torch.cat([_flat(B.unit(cond_u8)), torch.full((e,), CANARY_F)]).cuda(),
                dst=torch.full((2 * e,), CANARY_F, dtype=torch.float32, device="cuda"),
                scratch=torch.full((BP.scratch_bytes([(6, 7)]) + 256,), CANARY_B, dtype=torch.uint8, device="cuda"))
    before = {k: v.clone() for k, v in bufs.items()}
    off = (C.c_int64 * 1)(0)
    ok = dict(out=_p(bufs["out"]), cond=_p(bufs["cond"]), offs=off, hw=(C.c_int32 * 2)(6, 7), n=1, it=2, dst=_p(bufs["dst"]),
              scratch=_p(bufs["scratch"]))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.srgd_image_backproject_images(a["out"], a["cond"], a["offs"], a["hw"], a["n"], a["it"], a["dst"], a["scratch"], _stream())
        return rc, lib.srgd_image_backproject_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(bufs[k], before[k]) for k in bufs)
    at = lambda t, nbytes: C.c_void_p(t.data_ptr() + nbytes)      # noqa: E731
    refusals = [("null", dict(out=None)), ("null", dict(cond=None)), ("null", dict(offs=None)), ("null", dict(hw=None)),
                ("null", dict(dst=None)), ("null", dict(scratch=None)), ("n_images", dict(n=0)),
                ("iterations", dict(it=0)), ("iterations", dict(it=65)),
                ("bad size", dict(hw=(C.c_int32 * 2)(4, 7))), ("bad size", dict(hw=(C.c_int32 * 2)(6, 4))),
                ("2^31 - 256", dict(hw=(C.c_int32 * 2)(5, 8947848))), ("offset outside", dict(offs=(C.c_int64 * 1)(-4))),
                ("4-byte aligned", dict(out=at(bufs["out"], 2))), ("256-byte aligned", dict(scratch=at(bufs["scratch"], 64))),
                ("partial overlap of dst01 and out01", dict(dst=at(bufs["out"], 4))),
                ("partial overlap of dst01 and out01", dict(dst=at(bufs["out"], 4 * e - 4))),
                ("overlap of dst01 and cond01", dict(dst=_p(bufs["cond"]))), ("overlap of dst01 and cond01", dict(dst=at(bufs["cond"], 16)))]
    for word, kw in refusals:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
        assert untouched(), kw
    rc, msg = call()                                             # ... and the library is usable afterwards
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert np.array_equal(bufs["dst"][:e].view(3, 24, 28).cpu().numpy(), B.unit(seq[2])) and (bufs["dst"][e:] == CANARY_F).all()
    with pytest.raises(ValueError, match="do not fit"):          # the Python layer: buffers that do not fit
        BP.back_project_flat(bufs["out"][:e], bufs["cond"][:e], [0], [(24, 32)], 2)


# ------------------------------------------------------------------------------------------- 5. tiled_sample
E2E_SIZES = [(256, 256), (300, 500), (320, 480)]


def _run(sampler, seed, **kw):
    torch.manual_seed(seed)
    sampler.device_noise_seed = seed
    return sampler.tiled_sample(**kw)


def test_tiled_sample_back_project_on_the_mixed_list_path():
    from tests.test_engine_gpu import build_sampler
    sampler = build_sampler(16)
    g = torch.Generator().manual_seed(21)
    conds = [torch.rand(1, 3, h, w, generator=g).cuda() for (h, w) in E2E_SIZES]
    refs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for (h, w) in E2E_SIZES]
    kw = dict(batch_size=8, num_sample_steps=2, precision="bf16", class_label=torch.tensor([0, 2, 1]).cuda(), condition_x=conds)
    raw = _run(sampler, 5, **kw)
    assert all(torch.equal(a, b) for a, b in zip(_run(sampler, 5, back_project=0, **kw), raw))       # 0 is the call without the keyword
    got = _run(sampler, 5, back_project=3, **kw)
    want = INF.back_project_on_device(raw, conds, 3)
    assert all(a.shape == (1, 3) + s and torch.equal(a, b) for a, b, s in zip(got, want, E2E_SIZES))
    assert not any(torch.equal(a, b) for a, b in zip(got, raw))
    # after the colour fix, before the metrics
    fixed = _run(sampler, 5, color_fix="wavelet", **kw)
    outs, quality = _run(sampler, 5, color_fix="wavelet", reference=refs, back_project=3, **kw)
    assert all(torch.equal(a, b) for a, b in zip(outs, INF.back_project_on_device(fixed, conds, 3)))
    assert quality == MX.metrics_on_device(outs, refs) and quality != MX.metrics_on_device(fixed, refs)
    # per-image noise seeds: every sample is corrected against the same input
    seeded = _run(sampler, 123, seeds=[5, 9], back_project=3, **dict(kw, condition_x=[conds[1], conds[1]], class_label=torch.tensor([2, 2]).cuda()))
    assert torch.equal(seeded[0], got[1]) and not torch.equal(seeded[0], seeded[1])
    with pytest.raises(ValueError, match="bad image size"):      # before anything is sampled
        sampler.tiled_sample(**dict(kw, condition_x=torch.rand(1, 3, 300, 302).cuda(), class_label=None), back_project=3)


def test_tiled_sample_back_project_on_the_batch_path_trajectories_and_the_edm_wrapper():
    from tests.test_engine_gpu import build_edm_sampler, build_sampler
    sampler = build_sampler(16)
    g = torch.Generator().manual_seed(3)
    batch = torch.rand(2, 3, 300, 260, generator=g).cuda()
    ref = torch.randint(0, 256, (2, 300, 260, 3), generator=g, dtype=torch.uint8)
    kw = dict(batch_size=8, num_sample_steps=2, precision="fp32", class_label=torch.tensor([1]).cuda())
    raw = _run(sampler, 4, condition_x=batch, **kw)
    assert torch.equal(_run(sampler, 4, condition_x=batch, back_project=0, **kw), raw)
    got = _run(sampler, 4, condition_x=batch, back_project=3, **kw)
    assert got.shape == (2, 3, 300, 260) and torch.equal(got, INF.back_project_on_device(raw, batch, 3)) and not torch.equal(got, raw)
    fixed = _run(sampler, 4, condition_x=batch, color_fix="adain", **kw)
    out, quality = _run(sampler, 4, condition_x=batch, color_fix="adain", reference=list(ref), back_project=3, **kw)
    assert torch.equal(out, INF.back_project_on_device(fixed, batch, 3)) and quality == MX.metrics_on_device(out, ref)
    # trajectories stay raw: only the returned final image is corrected
    out_r, imgs_r, x0_r = _run(sampler, 4, condition_x=batch[:1], with_images=True, with_x0_images=True, **kw)
    out_b, imgs_b, x0_b = _run(sampler, 4, condition_x=batch[:1], with_images=True, with_x0_images=True, back_project=3, **kw)
    assert all(torch.equal(a, b) for a, b in zip(imgs_r, imgs_b)) and all(torch.equal(a, b) for a, b in zip(x0_r, x0_b))
    assert torch.equal(out_b, INF.back_project_on_device(out_r, batch[:1], 3)) and torch.equal(out_b, got[:1])
    # the EDM wrapper's [B,3,H,W] form
    edm = build_edm_sampler(16)
    ekw = dict(batch_size=8, num_sample_steps=2, precision="bf16", class_label=torch.tensor([0]).cuda())
    raw = _run(edm, 6, condition_x=batch, **ekw)
    assert torch.equal(_run(edm, 6, condition_x=batch, back_project=0, **ekw), raw)
    got = _run(edm, 6, condition_x=batch, back_project=3, **ekw)
    assert torch.equal(got, INF.back_project_on_device(raw, batch, 3)) and not torch.equal(got, raw)
    eout, eq = _run(edm, 6, condition_x=batch, color_fix="wavelet", reference=list(ref), back_project=3, **ekw)
    assert torch.equal(eout, INF.back_project_on_device(_run(edm, 6, condition_x=batch, color_fix="wavelet", **ekw), batch, 3))
    assert eq == MX.metrics_on_device(eout, ref)
    with pytest.raises(ValueError, match="bad image size"):
        edm.tiled_sample(condition_x=torch.rand(1, 3, 300, 302).cuda(), back_project=3, **ekw)
    assert "back_project" not in __import__("inspect").signature(sampler.sample).parameters     # un-tiled sample(): out of scope


# ------------------------------------------------------------------------------------------- 6. the command line
def test_cli_back_project_with_samples_and_consistency(tmp_path):
    from srgd_amd.synth import synth_state_dict
    from tests.test_engine_gpu import _schema
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    indir, outdir, plain = tmp_path / "in", tmp_path / "out", tmp_path / "plain"
    indir.mkdir()
    lr = np.random.default_rng(4).integers(0, 256, (40, 56, 3), dtype=np.uint8)
    Image.fromarray(lr, "RGB").save(indir / "a.png")
    base = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(indir),
            "--num_sample_steps", "2", "--test_label", "1", "--batch_size", "4", "--device_noise", "--seed", "71", "--samples", "2"]
    first = subprocess.run(base + ["--output_dir", str(plain)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert first.returncode == 0, first.stderr[-3000:]           # one child at a time
    names = ["a_out.png", "a_out_s1.png"]
    assert sorted(os.listdir(plain)) == names
    second = subprocess.run(base + ["--output_dir", str(outdir), "--back_project", "3", "--consistency"], cwd=ROOT, capture_output=True,
                            text=True, timeout=300)
    assert second.returncode == 0, second.stderr[-3000:]         # only after the first returned 0
    assert sorted(os.listdir(outdir)) == sorted(names + ["consistency.json"])
    png = lambda d, n: np.asarray(Image.open(d / n).convert("RGB"))              # noqa: E731
    cond = K.pillow_up(lr)
    doc = json.load(open(outdir / "consistency.json"))
    for n in names:                                              # every sample is corrected against the same input
        assert np.array_equal(png(outdir, n), B.steps(png(plain, n), cond, 3)[3]), n
        rec = K.yardstick(png(outdir, n), lr)[2]
        assert doc["files"][n] == rec
        assert rec["lr_mse"] < K.yardstick(png(plain, n), lr)[2]["lr_mse"], n
    assert not np.array_equal(png(outdir, names[0]), png(outdir, names[1]))
