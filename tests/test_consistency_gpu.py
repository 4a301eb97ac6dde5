"""LR consistency on the GPU (srgd_amd/csrc/consistency.hip, include/srgd_consistency.h) against Pillow itself
(tests/consistency_cases.py).  Inputs and outputs are 8-bit and every result is an integer: every comparison here is an equality
(``array_equal`` for the reduced output ``D``, ``==`` for the four integers and for the three float64 numbers the host derives from
them by the header's formulas).
LR sizes (h x w; a tile is 15 rows x 32 columns): 5x5 (every index a border row or the single interior one), 5x37, 37x5 and 6x7 (odd w:
the HR rows are not 16-byte aligned, guarded 4-byte loads), 8x8 (aligned, 16-byte loads), 16x33 (a full tile and a 1-pixel remainder
tile on each axis), 31x65 (two full tiles and a 1-pixel remainder both ways) and 300x300 for the 64-bit sums."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import consistency as CS
from srgd_amd import inference as INF
from tests import consistency_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
_cache = {}


def _case(kind, h, w):
    """(O, L, (D, integers, record) of the yardstick): computed once per session, shared, read-only."""
    key = (kind, h, w)
    if key not in _cache:
        if kind == "random":
            out, lr = K.random_pair(h, w, 7)
        elif kind == "overshoot":
            out, lr = K.overshoot_output(h, w), K.random_pair(h, w, 8)[1]
        else:                                                    # "up": O = Pillow x4 of L
            lr = K.random_pair(h, w, 9)[1]
            out = K.pillow_up(lr)
        out, lr = np.ascontiguousarray(out), np.ascontiguousarray(lr)
        out.setflags(write=False)
        lr.setflags(write=False)
        _cache[key] = (out, lr, K.yardstick(out, lr))
    return _cache[key]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _gpu(a):
    return torch.from_numpy(np.array(a)).cuda()


def _single(out, lr, with_down=True):
    """``srgd_image_consistency`` on one image; ``down`` is canary-filled beyond the image.  -> (D or None, four ints)."""
    h, w, _ = lr.shape
    e = 3 * h * w
    hr_t, lr_t = _gpu(out).reshape(-1), _gpu(lr).reshape(-1)
    down = torch.full((e + 64,), CANARY, dtype=torch.uint8, device="cuda") if with_down else None
    stats = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(CS.scratch_bytes([(h, w)]) // 8, dtype=torch.int64, device="cuda")
    rc = CS.lib().srgd_image_consistency(_p(hr_t), _p(lr_t), h, w, _p(down), _p(stats), _p(scratch),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, CS.lib().srgd_image_consistency_last_error()
    torch.cuda.synchronize()
    assert int(stats[4]) == -1 and (down is None or (down[e:] == CANARY).all())
    return (None if down is None else down[:e].view(h, w, 3).cpu().numpy()), tuple(stats[:4].cpu().tolist())


# ------------------------------------------------------------------------------------------- 1. both entries against Pillow
@pytest.mark.parametrize("h,w", K.SIZES)
def test_both_entries_equal_pillow(h, w):
    kinds = ["random", "up"] + (["overshoot"] if (h, w) in K.OVERSHOOT_SIZES else [])
    cases = [_case(kind, h, w) for kind in kinds]
    for kind, (out, lr, (down, ints, rec)) in zip(kinds, cases):
        got_down, got_ints = _single(out, lr)
        print(f"{kind} {h}x{w}: integers {got_ints} (Pillow {ints}), D differs in {int((got_down != down).sum())} bytes")
        assert np.array_equal(got_down, down), kind
        assert got_ints == ints, kind
        assert _single(out, lr, with_down=False) == (None, ints), kind
    got = CS.consistency_on_device([_gpu(c[0]) for c in cases], [_gpu(c[1]) for c in cases], return_down=True)     # ONE batched call
    assert len(got) == len(cases)
    for (out, lr, (down, ints, rec)), (got_rec, got_down) in zip(cases, got):
        assert got_down.dtype == torch.uint8 and tuple(got_down.shape) == lr.shape and np.array_equal(got_down.cpu().numpy(), down)
        assert got_rec == rec
    one = CS.consistency_on_device(_gpu(cases[0][0]), _gpu(cases[0][1]))       # the tensor form: one dict, no D
    assert one == cases[0][2][2] and list(one) == list(K.KEYS)


def test_constant_images_and_the_64_bit_sums():
    for v in (0, 77, 255):
        down, ints = _single(K.constant(32, 28, v), K.constant(8, 7, v))
        assert (down == v).all() and ints == (0, 0, 0, 0)
    rec = CS.consistency_on_device(_gpu(K.constant(32, 28, 77)), _gpu(K.constant(8, 7, 77)))
    assert rec == {"lr_psnr": math.inf, "lr_mse": 0.0, "lr_max_abs": 0.0}
    # O all 255 against L all 0 at 300 x 300: 255^2 * 90,000 per channel = 5,852,250,000 > 2^32
    down, ints = _single(K.constant(1200, 1200, 255), K.constant(300, 300, 0))
    assert (down == 255).all() and ints == (255 * 255 * 90000,) * 3 + (255,) and ints[0] > 2 ** 32
    rec = CS.consistency_on_device(_gpu(K.constant(1200, 1200, 255)), _gpu(K.constant(300, 300, 0)))
    assert rec == {"lr_psnr": 0.0, "lr_mse": 65025.0, "lr_max_abs": 255.0}


# ------------------------------------------------------------------------------------------- 2. alone, in a group, at any offset
def _group(items, gaps, with_down=True):
    """``items`` = [(O, L)] laid out in order with ``gaps[j]`` (multiples of 16) canary bytes in front of image j in every buffer.
    -> per image (D or None, four ints); asserts that every canary byte - gaps, padding, tails - is untouched."""
    sizes = [lr.shape[:2] for _, lr in items]
    h_offs, l_offs, h_tot, l_tot = [], [], 0, 0
    for (out, lr), gap in zip(items, gaps):
        h_tot += gap
        l_tot += 2 * gap
        h_offs.append(h_tot)
        l_offs.append(l_tot)
        h_tot += CS.padded(out.size)
        l_tot += CS.padded(lr.size)
    hr = torch.full((h_tot + 32,), CANARY, dtype=torch.uint8)
    lo = torch.full((l_tot + 32,), CANARY, dtype=torch.uint8)
    for (out, lr), ho, loff in zip(items, h_offs, l_offs):
        hr[ho:ho + out.size] = torch.from_numpy(np.array(out)).reshape(-1)
        lo[loff:loff + lr.size] = torch.from_numpy(np.array(lr)).reshape(-1)
    hr_host, lo_host = hr.clone(), lo.clone()
    hr, lo = hr.cuda(), lo.cuda()
    down = torch.full((l_tot + 32,), CANARY, dtype=torch.uint8, device="cuda") if with_down else None
    stats = CS.consistency_flat_device(hr, h_offs, lo, l_offs, sizes, down, l_offs if with_down else None)
    torch.cuda.synchronize()
    assert torch.equal(hr.cpu(), hr_host) and torch.equal(lo.cpu(), lo_host)           # inputs are read only
    res, used = [], torch.zeros(l_tot + 32, dtype=torch.bool, device="cuda")
    for i, ((out, lr), loff) in enumerate(zip(items, l_offs)):
        h, w, _ = lr.shape
        used[loff:loff + lr.size] = True
        res.append((down[loff:loff + lr.size].view(h, w, 3).cpu().numpy() if with_down else None, tuple(stats[i].cpu().tolist())))
    assert down is None or (down[~used] == CANARY).all()         # gaps and the padding of down_u8 come back untouched
    return res


def test_an_image_is_bit_identical_alone_in_a_group_and_at_any_offset():
    shapes = [(5, 5), (5, 37), (6, 7), (8, 8), (K.TILE_H + 1, K.TILE_W + 1), (2 * K.TILE_H + 1, 2 * K.TILE_W + 1)]
    items = [_case("random", h, w)[:2] for (h, w) in shapes]
    alone = [_single(out, lr) for out, lr in items]
    for (h, w), got in zip(shapes, alone):
        down, ints, _ = _case("random", h, w)[2]
        assert np.array_equal(got[0], down) and got[1] == ints
    order = [3, 5, 0, 2, 4, 1]
    layouts = [(list(range(6)), _group(items, [0] * 6)),
               (order, _group([items[i] for i in order], [16, 48, 1024, 0, 4096, 160])),
               (order[::-1], _group([items[i] for i in order[::-1]], [4112, 16, 0, 32, 16, 16], with_down=False))]
    for idx, got in layouts:
        for pos, i in enumerate(idx):
            assert got[pos][1] == alone[i][1], (idx, i)
            assert got[pos][0] is None or np.array_equal(got[pos][0], alone[i][0]), (idx, i)
    # the same image twice in one call, at two different offsets
    twice = _group([items[4], items[1], items[4]], [32, 0, 80])
    assert twice[0][1] == twice[2][1] == alone[4][1] and np.array_equal(twice[0][0], twice[2][0]) and np.array_equal(twice[0][0], alone[4][0])


# ------------------------------------------------------------------------------------------- 3. more than 128 images
def test_more_than_128_images_in_one_call():
    n = 131
    pairs = [K.random_pair(5, 5, 500 + i) for i in range(n)]
    got = CS.consistency_on_device([_gpu(o) for o, _ in pairs], [_gpu(l) for _, l in pairs], return_down=True)
    assert len(got) == n
    for i, ((out, lr), (rec, down)) in enumerate(zip(pairs, got)):
        want_down, _, want = K.yardstick(out, lr)
        assert np.array_equal(down.cpu().numpy(), want_down) and rec == want, i


# ------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_write_nothing_and_leave_the_library_usable():
    lib = CS.lib()
    out, lr, (down, ints, _) = _case("random", 6, 7)
    hr_t, lr_t = _gpu(out).reshape(-1), _gpu(lr).reshape(-1)
    bufs = dict(down=torch.full((256,), CANARY, dtype=torch.uint8, device="cuda"),
                stats=torch.full((4,), -1, dtype=torch.int64, device="cuda"),
                scratch=torch.full((4,), -1, dtype=torch.int64, device="cuda"))
    off = (C.c_int64 * 1)(0)
    ok = dict(hr=_p(hr_t), hr_offs=off, lr=_p(lr_t), lr_offs=off, hw=(C.c_int32 * 2)(6, 7), n=1, down=_p(bufs["down"]), down_offs=off,
              stats=_p(bufs["stats"]), scratch=_p(bufs["scratch"]))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.srgd_image_consistency_images(a["hr"], a["hr_offs"], a["lr"], a["lr_offs"], a["hw"], a["n"], a["down"], a["down_offs"],
                                               a["stats"], a["scratch"], st)
        return rc, lib.srgd_image_consistency_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return bool((bufs["down"] == CANARY).all() and (bufs["stats"] == -1).all() and (bufs["scratch"] == -1).all())
    refusals = [("null", dict(hr=None)), ("null", dict(lr=None)), ("null", dict(hw=None)), ("null", dict(stats=None)),
                ("null", dict(scratch=None)), ("null", dict(hr_offs=None)), ("null", dict(lr_offs=None)),
                ("together", dict(down=None)), ("together", dict(down_offs=None)),
                ("n_images", dict(n=0)), ("bad size", dict(hw=(C.c_int32 * 2)(4, 7))), ("bad size", dict(hw=(C.c_int32 * 2)(6, 4))),
                ("2^31 - 256", dict(hw=(C.c_int32 * 2)(5, 8947848))),
                ("misaligned offset", dict(hr_offs=(C.c_int64 * 1)(8))), ("misaligned offset", dict(down_offs=(C.c_int64 * 1)(4))),
                ("offset outside", dict(lr_offs=(C.c_int64 * 1)(-16))),
                ("16-byte aligned", dict(hr=C.c_void_p(hr_t.data_ptr() + 4))),
                ("8-byte aligned", dict(stats=C.c_void_p(bufs["stats"].data_ptr() + 4)))]
    for word, kw in refusals:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
        assert untouched(), kw
    rc, msg = call()                                             # ... and the library is usable afterwards
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert np.array_equal(bufs["down"][:lr.size].view(6, 7, 3).cpu().numpy(), down) and (bufs["down"][lr.size:] == CANARY).all()
    assert tuple(bufs["stats"].cpu().tolist()) == ints
    with pytest.raises(ValueError, match="do not fit"):          # the Python layer: buffers that do not fit
        CS.consistency_flat(hr_t, [0], lr_t, [0], [(6, 8)])


# ------------------------------------------------------------------------------------------- 5. the command line
def test_cli_consistency_with_samples_and_ensemble(tmp_path):
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
            "--num_sample_steps", "2", "--test_label", "1", "--batch_size", "4", "--device_noise", "--seed", "71", "--samples", "2",
            "--ensemble"]
    first = subprocess.run(base + ["--output_dir", str(outdir), "--consistency"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert first.returncode == 0, first.stderr[-3000:]           # one child at a time
    names = ["a_out.png", "a_out_mean.png", "a_out_s1.png", "a_out_std.png", "ensemble.json"]
    assert sorted(os.listdir(outdir)) == sorted(names + ["consistency.json"])
    png = lambda n: np.asarray(Image.open(outdir / n).convert("RGB"))           # noqa: E731
    want = {n: K.yardstick(png(n), lr)[2] for n in ("a_out.png", "a_out_s1.png", "a_out_mean.png")}
    doc = json.load(open(outdir / "consistency.json"))
    assert list(doc) == ["files", "images", "mean", "ensemble", "ensemble_mean"]
    assert doc["files"] == {"a_out.png": want["a_out.png"], "a_out_s1.png": want["a_out_s1.png"]}
    assert want["a_out.png"] != want["a_out_s1.png"] and all(math.isfinite(v) for r in want.values() for v in r.values())
    mean = {k: (want["a_out.png"][k] + want["a_out_s1.png"][k]) / 2 for k in K.KEYS}
    assert doc["images"] == {"a.png": mean} and doc["mean"] == mean
    assert doc["ensemble"] == {"a.png": want["a_out_mean.png"]} and doc["ensemble_mean"] == want["a_out_mean.png"]
    # the same run without the flag on a fresh directory: no consistency.json, every other file byte for byte the same
    second = subprocess.run(base + ["--output_dir", str(plain)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert second.returncode == 0, second.stderr[-3000:]         # only after the first returned 0
    assert sorted(os.listdir(plain)) == sorted(names)
    for n in names:
        assert open(plain / n, "rb").read() == open(outdir / n, "rb").read(), n
