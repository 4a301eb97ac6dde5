"""The ensemble on the GPU (srgd_amd/csrc/ensemble.hip, include/srgd_ensemble.h) against the integer yardstick of
tests/ensemble_cases.py.  Every comparison is exact (``array_equal``) but ``mean_std``, the one sum of floats, which is within
1e-9 absolute: the test shapes have at most 12,288 elements, every term is at most 127.5 in 8-bit units, and 12,288 float64
additions of partial sums of at most 12,288 * 127.5 err by less than 12,288 * 2^-53 * 127.5 ~ 1.8e-10 (below 1e-11 for the kernels'
pairwise order); the derivation is in tests/ensemble_cases.py.
Shapes: 5x7 (105 bytes: six full 16-byte vectors and a tail of 9), 16x16 (768: no tail), 20x37 (2,220: more than two waves, tail of
12), 1x1 (a tail alone), 37x37 (4,107: one chunk of 4,096 and a second one that is a tail alone) and 64x64 (12,288: three chunks)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import ensemble as EN
from srgd_amd import inference as INF
from srgd_amd import metrics as MX
from tests import ensemble_cases as E
from tests import metrics_cases as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(5, 7), (16, 16), (20, 37), (1, 1), (37, 37), (64, 64)]
KS = [2, 3, 5, 7, 64, 256]
SENTINEL = 0xA5
_cache = {}


def _case(kind, k, h, w):
    """(samples uint8 [K,h,w,3], (mean, spread, stats) of the yardstick): computed once per session, shared, read-only."""
    key = (kind, k, h, w)
    if key not in _cache:
        x = {"random": lambda: E.random_samples(k, h, w, 1000 * k + 10 * h + w), "all_means": lambda: E.all_means_samples(k, 7),
             "extreme": lambda: E.extreme_samples(k, h, w, k)}[kind]()
        x.setflags(write=False)
        _cache[key] = (x, E.restate(x))
    return _cache[key]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _padded_flat(x):
    """uint8 [K,h,w,3] -> the flat sample buffer of the C entries (stride padded to 16, padding = sentinel) on the GPU."""
    k, e = x.shape[0], x[0].size
    flat = np.full((k, EN.padded(e)), SENTINEL, dtype=np.uint8)
    flat[:, :e] = x.reshape(k, e)
    return torch.from_numpy(flat.reshape(-1)).cuda()


def _single(x, with_mean01=True):
    """``srgd_image_ensemble`` on one image; outputs are sentinel-filled beyond the image.  -> (mean, std, stats, mean01 or None)."""
    k, h, w, _ = x.shape
    e = 3 * h * w
    flat = _padded_flat(x)
    mean = torch.full((EN.padded(e) + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    std = torch.full_like(mean, SENTINEL)
    m01 = torch.full((e + 8,), -7.0, dtype=torch.float32, device="cuda") if with_mean01 else None
    stats = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    scratch = torch.empty(EN.scratch_doubles([(h, w)]), dtype=torch.float64, device="cuda")
    rc = EN.lib().srgd_image_ensemble(_p(flat), k, h, w, _p(mean), _p(std), _p(m01), _p(stats), _p(scratch),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, EN.lib().srgd_image_ensemble_last_error()
    torch.cuda.synchronize()
    assert (mean[e:] == SENTINEL).all() and (std[e:] == SENTINEL).all() and (m01 is None or (m01[e:] == -7.0).all())
    return (mean[:e].view(h, w, 3).cpu().numpy(), std[:e].view(h, w, 3).cpu().numpy(), stats.cpu().tolist(),
            None if m01 is None else m01[:e].view(3, h, w).cpu().numpy())


def _check(got_mean, got_std, got_stats, want, tag):
    mean, std, stats = want
    assert np.array_equal(got_mean, mean), tag
    assert np.array_equal(got_std, std), tag
    mean_std, max_std = (got_stats["mean_std"], got_stats["max_std"]) if isinstance(got_stats, dict) else got_stats
    print(f"{tag}: mean_std {mean_std!r} (yardstick {stats['mean_std']!r}, diff {mean_std - stats['mean_std']:.3e}), max_std {max_std!r}")
    assert max_std == stats["max_std"], tag                      # exact: an integer maximum, one square root, one division
    assert abs(mean_std - stats["mean_std"]) <= E.MEAN_STD_TOL, tag


# ------------------------------------------------------------------------------------------- 1. both entries against the yardstick
@pytest.mark.parametrize("k", KS)
def test_both_entries_equal_the_yardstick(k):
    cases = [_case("random", k, h, w) for (h, w) in SIZES] + [_case("all_means", k, 16, 16), _case("extreme", k, 20, 37)]
    for x, want in cases:
        mean, std, stats, m01 = _single(x)
        _check(mean, std, stats, want, f"single K={k} {x.shape[1]}x{x.shape[2]}")
        assert np.array_equal(m01.view(np.uint32), E.mean01(want[0]).view(np.uint32))
    assert len(np.unique(cases[-2][1][0])) == 256                # the mean image of that case takes all 256 values
    assert set(np.unique(cases[-1][0])) == {0, 255}
    got = EN.ensemble_on_device([torch.from_numpy(x).cuda() for x, _ in cases], return_mean01=True)     # ONE batched call
    assert len(got) == len(cases)
    for (x, want), (mean, std, stats, m01) in zip(cases, got):
        assert mean.dtype == torch.uint8 and tuple(mean.shape) == x.shape[1:] == tuple(std.shape) and tuple(m01.shape) == (1, 3) + x.shape[1:3]
        _check(mean.cpu().numpy(), std.cpu().numpy(), stats, want, f"group K={k} {x.shape[1]}x{x.shape[2]}")
        assert np.array_equal(m01[0].cpu().numpy().view(np.uint32), E.mean01(want[0]).view(np.uint32))
    one = EN.ensemble_on_device(torch.from_numpy(cases[2][0]).cuda())         # the tensor form: one tuple, no mean01
    assert len(one) == 3 and np.array_equal(one[0].cpu().numpy(), cases[2][1][0]) and np.array_equal(one[1].cpu().numpy(), cases[2][1][1])


# ------------------------------------------------------------------------------------------- 2. mean01
def test_mean01_is_what_to_tensor_reads_back_and_a_null_pointer_writes_nothing():
    x, want = _case("all_means", 5, 16, 16)
    mean, std, stats, m01 = _single(x)
    assert np.array_equal(m01.view(np.uint32), (want[0].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1).view(np.uint32))
    back = INF.unit_tensor_to_u8_on_device(torch.from_numpy(m01).cuda())      # the engine's own (int)(x * 255.0f)
    assert np.array_equal(back.cpu().numpy(), want[0]) and len(np.unique(want[0])) == 256
    for x, want in (_case("random", 3, 20, 37), _case("random", 7, 37, 37)):
        with_m01, without = _single(x), _single(x, with_mean01=False)
        assert without[3] is None and np.array_equal(with_m01[0], without[0]) and np.array_equal(with_m01[1], without[1])
        assert with_m01[2] == without[2]
        back = INF.unit_tensor_to_u8_on_device(torch.from_numpy(with_m01[3]).cuda())
        assert np.array_equal(back.cpu().numpy(), want[0])
    # the group entry with a null mean01: a sentinel-filled buffer that is not handed over stays as it is (and so do the others)
    got = EN.ensemble_on_device([torch.from_numpy(_case("random", 3, 20, 37)[0]).cuda()])
    assert len(got[0]) == 3


# ------------------------------------------------------------------------------------------- 3. alone, in a group, at any offset
def _group(images, order, gaps, k, with_mean01=True):
    """The images in ``order`` with ``gaps[j]`` (multiples of 16) sentinel bytes in front of image j, in sentinel-filled buffers.
    -> per image (mean, std, stats, mean01) in the ORIGINAL order; asserts that everything outside the images is untouched."""
    n = len(images)
    s_offs, o_offs, m_offs, s_tot, o_tot, m_tot = [0] * n, [0] * n, [0] * n, 0, 0, 0
    for j, i in enumerate(order):
        e = images[i][0].size
        s_tot += gaps[j]
        o_tot += 2 * gaps[j]
        m_tot += gaps[j] // 16 + j                               # mean01 offsets need no alignment
        s_offs[i], o_offs[i], m_offs[i] = s_tot, o_tot, m_tot
        s_tot += k * EN.padded(e)
        o_tot += EN.padded(e)
        m_tot += e
    samples = torch.full((s_tot + 32,), SENTINEL, dtype=torch.uint8)
    for i, x in enumerate(images):
        e = x[0].size
        for j in range(k):
            samples[s_offs[i] + j * EN.padded(e):s_offs[i] + j * EN.padded(e) + e] = torch.from_numpy(x[j].reshape(-1))
    samples = samples.cuda()
    mean = torch.full((o_tot + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    std = torch.full_like(mean, SENTINEL)
    m01 = torch.full((m_tot + 8,), -7.0, dtype=torch.float32, device="cuda") if with_mean01 else None
    sizes = [x.shape[1:3] for x in images]
    stats = EN.ensemble_flat_device(samples, s_offs, sizes, k, mean, std, o_offs, m01, m_offs if with_mean01 else None)
    torch.cuda.synchronize()
    out, used, used01 = [], torch.zeros_like(mean, dtype=torch.bool), torch.zeros(m_tot + 8, dtype=torch.bool, device="cuda")
    for i, x in enumerate(images):
        e, (h, w) = x[0].size, x.shape[1:3]
        used[o_offs[i]:o_offs[i] + e] = True
        used01[m_offs[i]:m_offs[i] + e] = True
        out.append((mean[o_offs[i]:o_offs[i] + e].view(h, w, 3).cpu().numpy(), std[o_offs[i]:o_offs[i] + e].view(h, w, 3).cpu().numpy(),
                    stats[i].cpu().tolist(), m01[m_offs[i]:m_offs[i] + e].view(3, h, w).cpu().numpy() if with_mean01 else None))
    assert (mean[~used] == SENTINEL).all() and (std[~used] == SENTINEL).all()          # padding and gaps come back untouched
    assert m01 is None or (m01[~used01] == -7.0).all()
    return out


def test_an_image_is_bit_identical_alone_in_a_group_and_at_any_offset():
    k = 3
    images = [_case("random", k, h, w)[0] for (h, w) in ((5, 7), (37, 37), (20, 37))]
    alone = [_single(x) for x in images]
    for i, x in enumerate(images):
        _check(alone[i][0], alone[i][1], alone[i][2], _case("random", k, *x.shape[1:3])[1], f"alone {i}")
    layouts = [_group(images, [0, 1, 2], [0, 0, 0], k), _group(images, [2, 0, 1], [16, 48, 1024], k),
               _group(images, [1, 2, 0], [4096, 16, 160], k, with_mean01=False)]
    solo_at_offset = [_group([x], [0], [gap], k)[0] for x, gap in zip(images, (32, 0, 4112))]
    for got in layouts + [solo_at_offset]:
        for i in range(len(images)):
            assert np.array_equal(got[i][0], alone[i][0]) and np.array_equal(got[i][1], alone[i][1]), i
            assert got[i][2] == alone[i][2], i                   # both doubles, bit for bit
            assert got[i][3] is None or np.array_equal(got[i][3].view(np.uint32), alone[i][3].view(np.uint32)), i


# ------------------------------------------------------------------------------------------- 4. more than 128 images
def test_more_than_128_images_in_one_call():
    n, k = 131, 2
    xs = [E.random_samples(k, 3, 5, 500 + i) for i in range(n)]
    got = EN.ensemble_on_device([torch.from_numpy(x).cuda() for x in xs], return_mean01=True)
    assert len(got) == n
    for i, (x, (mean, std, stats, m01)) in enumerate(zip(xs, got)):
        want = E.restate(x)
        assert np.array_equal(mean.cpu().numpy(), want[0]) and np.array_equal(std.cpu().numpy(), want[1]), i
        assert stats["max_std"] == want[2]["max_std"] and abs(stats["mean_std"] - want[2]["mean_std"]) <= E.MEAN_STD_TOL, i
        assert np.array_equal(m01[0].cpu().numpy().view(np.uint32), E.mean01(want[0]).view(np.uint32)), i


# ------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_write_nothing_and_leave_the_library_usable():
    lib = EN.lib()
    x, want = _case("random", 3, 5, 7)
    k, h, w = 3, 5, 7
    e = 3 * h * w
    flat = _padded_flat(x)
    bufs = dict(mean=torch.full((256,), SENTINEL, dtype=torch.uint8, device="cuda"),
                std=torch.full((256,), SENTINEL, dtype=torch.uint8, device="cuda"),
                m01=torch.full((e + 8,), -7.0, dtype=torch.float32, device="cuda"),
                stats=torch.full((2,), -1.0, dtype=torch.float64, device="cuda"),
                scratch=torch.full((4,), -1.0, dtype=torch.float64, device="cuda"))
    off = (C.c_int64 * 1)(0)
    ok = dict(samples=_p(flat), offs=off, hw=(C.c_int32 * 2)(h, w), n=1, k=k, mean=_p(bufs["mean"]), std=_p(bufs["std"]), out=off,
              m01=_p(bufs["m01"]), m01_offs=off, stats=_p(bufs["stats"]), scratch=_p(bufs["scratch"]))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.srgd_image_ensemble_images(a["samples"], a["offs"], a["hw"], a["n"], a["k"], a["mean"], a["std"], a["out"], a["m01"],
                                            a["m01_offs"], a["stats"], a["scratch"], st)
        return rc, lib.srgd_image_ensemble_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return bool((bufs["mean"] == SENTINEL).all() and (bufs["std"] == SENTINEL).all() and (bufs["m01"] == -7.0).all()
                    and (bufs["stats"] == -1.0).all() and (bufs["scratch"] == -1.0).all())
    refusals = [("null", dict(samples=None)), ("null", dict(offs=None)), ("null", dict(hw=None)), ("null", dict(mean=None)),
                ("null", dict(std=None)), ("null", dict(out=None)), ("null", dict(stats=None)), ("null", dict(scratch=None)),
                ("together", dict(m01_offs=None)), ("together", dict(m01=None)),
                ("n_images", dict(n=0)), ("n_images", dict(n=-3)),
                ("n_samples", dict(k=1)), ("n_samples", dict(k=257)),
                ("bad size", dict(hw=(C.c_int32 * 2)(0, w))), ("bad size", dict(hw=(C.c_int32 * 2)(h, 0))),
                ("2^31 - 256", dict(hw=(C.c_int32 * 2)(1, 715827798))),
                ("misaligned offset", dict(offs=(C.c_int64 * 1)(8))), ("misaligned offset", dict(out=(C.c_int64 * 1)(4))),
                ("offset outside", dict(offs=(C.c_int64 * 1)(-16))),
                ("16-byte aligned", dict(samples=C.c_void_p(flat.data_ptr() + 4))),
                ("16-byte aligned", dict(mean=C.c_void_p(bufs["mean"].data_ptr() + 8)))]
    for word, kw in refusals:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
        assert untouched(), kw
    rc = lib.srgd_image_ensemble(_p(flat), 1, h, w, ok["mean"], ok["std"], None, ok["stats"], ok["scratch"], st)
    assert rc == -1 and "n_samples" in lib.srgd_image_ensemble_last_error().decode() and untouched()
    rc, msg = call()                                             # ... and the library is usable afterwards
    assert rc == 0, msg
    torch.cuda.synchronize()
    _check(bufs["mean"][:e].view(h, w, 3).cpu().numpy(), bufs["std"][:e].view(h, w, 3).cpu().numpy(), bufs["stats"].cpu().tolist(), want,
           "after the refusals")
    assert (bufs["mean"][e:] == SENTINEL).all() and (bufs["std"][e:] == SENTINEL).all() and (bufs["m01"][e:] == -7.0).all()
    # the Python layer: buffers that do not fit, a K outside the range
    with pytest.raises(ValueError, match="do not fit"):
        EN.ensemble_flat(flat, [0], [(h, w + 1)], k, bufs["mean"], bufs["std"], [0])
    with pytest.raises(ValueError, match="number of samples"):
        EN.ensemble_flat(flat, [0], [(h, w)], 1, bufs["mean"], bufs["std"], [0])


# ------------------------------------------------------------------------------------------- 6. the mean image's PSNR / SSIM
def test_the_mean_image_goes_through_the_metrics_as_its_png_would():
    x, want = _case("random", 5, 20, 37)
    ref = np.random.default_rng(9).integers(0, 256, (20, 37, 3), dtype=np.uint8)
    mean, _, _, m01 = EN.ensemble_on_device(torch.from_numpy(x).cuda(), return_mean01=True)
    got = MX.metrics_on_device(m01, torch.from_numpy(ref), crop_border=4)[0]
    flat = MX.metrics_flat(m01.reshape(-1), torch.from_numpy(ref).cuda().reshape(-1), [0], [0], [(20, 37)], 4)[0]
    assert got == flat
    yard = M.restate_u8(want[0].astype(np.int64), ref, 4)        # the metrics' yardstick on the yardstick's mean image
    for key in M.KEYS:
        assert M.same_kind_or_close(got[key], yard[key]), (key, got[key], yard[key])


# ------------------------------------------------------------------------------------------- 7. the command line
def test_cli_ensemble_and_its_resumed_run(tmp_path):
    from srgd_amd.synth import synth_state_dict
    from tests.test_engine_gpu import _schema
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    indir, outdir = tmp_path / "in", tmp_path / "out"
    indir.mkdir()
    Image.fromarray(np.random.default_rng(4).integers(0, 256, (40, 56, 3), dtype=np.uint8), "RGB").save(indir / "a.png")
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(indir),
           "--output_dir", str(outdir), "--num_sample_steps", "2", "--test_label", "1", "--batch_size", "4", "--device_noise",
           "--seed", "71", "--samples", "3", "--ensemble"]
    names = ["a_out.png", "a_out_mean.png", "a_out_s1.png", "a_out_s2.png", "a_out_std.png", "ensemble.json"]
    first = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)           # one child at a time
    assert first.returncode == 0, first.stderr[-3000:]
    assert sorted(os.listdir(outdir)) == names
    before = {n: open(outdir / n, "rb").read() for n in names}
    png = lambda n: np.asarray(Image.open(outdir / n).convert("RGB"))                               # noqa: E731
    stack = np.stack([png(INF.sample_output_name("a.png", k)) for k in range(3)])
    assert stack.shape == (3, 160, 224, 3) and not np.array_equal(stack[0], stack[1])
    mean, std, stats = E.restate(stack)
    assert np.array_equal(png("a_out_mean.png"), mean) and np.array_equal(png("a_out_std.png"), std)
    doc = json.loads(before["ensemble.json"])
    rec = doc["files"]["a.png"]
    assert doc["samples"] == 3 and list(doc["files"]) == ["a.png"] and rec["mean"] == "a_out_mean.png" and rec["std"] == "a_out_std.png"
    assert rec["max_std"] == stats["max_std"] and doc["mean_std"] == rec["mean_std"]
    # 107,520 elements here: a term passes through at most 16 (its lane) + 6 (wave) + 2 (workgroup) + 1 + 8 (the 27 records) = 33
    # additions in the kernels' order, each erring by at most 2^-53 of a partial sum: below 33 * 2^-53 * 127.5 ~ 5e-13 in 8-bit units
    assert abs(rec["mean_std"] - stats["mean_std"]) <= E.MEAN_STD_TOL
    # the same command after one sample and both ensemble files are gone: only that sample is drawn, every file comes back
    for n in ("a_out_s1.png", "a_out_mean.png", "a_out_std.png"):
        os.remove(outdir / n)
    second = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)          # only after the first returned 0
    assert second.returncode == 0, second.stderr[-3000:]
    assert second.stdout.splitlines().count("skip") == 2         # skip-if-exists: the two samples found on disk
    assert {n: open(outdir / n, "rb").read() for n in sorted(os.listdir(outdir))} == before
