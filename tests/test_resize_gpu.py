"""srgd_amd.resize on the MI355X: every case, filter and pattern of tests/resize_cases.py against the numpy restatement as equality,
each destination inside a larger sentinel-filled buffer whose other bytes must not change; groups against solo calls; the 128-image
boundary of a launch sequence; the refusals with real buffers; the list API; and --outscale on the command line.

Pillow is imported for reading and writing PNG files only: the comparison target is the restatement, which
tests/test_resize_cpu.py pins against Pillow itself.  (16,16)->(1,1) of the case table is 16 : 1, outside the geometry the library
accepts: here it is one of the refusals.  The command-line test samples a 22x24 and a 24x22 input: a side of 20 pixels is refused
by the tiling of the sampler itself (a reflect pad of 88 rows on the 80 rows of its x4 image, as upstream), with or without
--outscale, so 22 is the smallest side next to 24 that can be sampled."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import resize as RZ
from tests import resize_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5


def _round(n):
    return (n + 15) // 16 * 16


def _call(items, filter, order=None, lead=48, gap=32):
    """One ``resize_flat`` call on ``items`` = ``[(uint8 [h,w,3] array, (h_out, w_out))]``.  The destination images lie in ``order``
    (default: as given) in a sentinel-filled buffer, ``lead`` bytes in front of the first and at least ``gap`` bytes between two.
    -> (results in the order of ``items``, the whole destination buffer, the mask of its bytes that belong to an image)."""
    order = list(range(len(items))) if order is None else order
    src_offsets, at = [], 0
    for img, _ in items:
        src_offsets.append(at)
        at += _round(img.size) + 16
    src = np.full(at, 0x3C, np.uint8)
    for (img, _), off in zip(items, src_offsets):
        src[off:off + img.size] = img.reshape(-1)
    dst_offsets, at = [0] * len(items), lead
    for i in order:
        dst_offsets[i] = at
        at += _round(3 * items[i][1][0] * items[i][1][1]) + gap
    dst = torch.full((at,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = [img.shape[:2] + tuple(out) for img, out in items]
    RZ.resize_flat(torch.from_numpy(src).cuda(), src_offsets, dst, dst_offsets, sizes, filter)
    torch.cuda.synchronize()
    whole = dst.cpu().numpy()
    inside = np.zeros(at, bool)
    results = []
    for (_, (h, w)), off in zip(items, dst_offsets):
        inside[off:off + 3 * h * w] = True
        results.append(whole[off:off + 3 * h * w].reshape(h, w, 3))
    return results, whole, inside


# ------------------------------------------------------------------------------------------- (a) the kernels are the restatement
@pytest.mark.parametrize("filter", list(RC.FILTERS))
def test_every_case_is_the_restatement_bit_for_bit_and_nothing_else_is_written(filter):
    assert len(RC.DEVICE_CASES) >= 20
    for in_size, out_size in RC.DEVICE_CASES:
        for name in RC.PATTERNS:
            (got,), whole, inside = _call([(RC.pattern(name, *in_size), out_size)], filter)
            want = RC.expected(name, in_size, out_size, filter)
            assert got.shape == want.shape and np.array_equal(got, want), (in_size, out_size, filter, name, int((got != want).sum()))
            assert (~inside).sum() >= 80 and (whole[~inside] == SENTINEL).all(), (in_size, out_size, filter, name)


def test_every_image_of_a_group_is_its_solo_call():
    picks = [((129, 67), (43, 100)), ((33, 65), (33, 31)), ((8, 6), (64, 48)), ((5, 7), (5, 7))]     # both passes, one, upscale, copy
    assert all(case in RC.DEVICE_CASES for case in picks)
    for filter in RC.FILTERS:
        items = [(RC.pattern("noise", *a), b) for a, b in picks]
        grouped, whole, inside = _call(items, filter, order=[2, 0, 3, 1], lead=16, gap=80)
        assert (whole[~inside] == SENTINEL).all()
        for item, (a, b), got in zip(items, picks, grouped):
            (solo,), _, _ = _call([item], filter, lead=0)
            assert np.array_equal(got, solo) and np.array_equal(got, RC.expected("noise", a, b, filter)), (a, b, filter)


def test_a_group_of_130_crosses_the_launch_sequence_boundary():
    in_size, out_size = RC.SMALLEST
    rng = np.random.default_rng(7)
    images = [rng.integers(0, 256, in_size + (3,), dtype=np.uint8) for _ in range(130)]
    grouped, whole, inside = _call([(img, out_size) for img in images], "bicubic")
    assert (whole[~inside] == SENTINEL).all()
    for i, (img, got) in enumerate(zip(images, grouped)):
        if i in (0, 1, 63, 127, 128, 129):                                    # solo calls on both sides of the boundary
            (solo,), _, _ = _call([(img, out_size)], "bicubic")
            assert np.array_equal(got, solo), i
        assert np.array_equal(got, RC.resize_u8(img, out_size[0], out_size[1], "bicubic")), i


def test_the_list_api_moves_images_to_the_gpu_and_returns_device_tensors():
    picks = [((40, 52), (20, 26)), ((40, 52), (30, 39)), ((37, 23), (23, 37))]
    images = [torch.from_numpy(RC.pattern("noise", *a).copy()) for a, _ in picks]
    images[1] = images[1].cuda()
    outs = RZ.resize_on_device(images, [b for _, b in picks], "lanczos")
    for (a, b), out in zip(picks, outs):
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == b + (3,)
        assert np.array_equal(out.cpu().numpy(), RC.expected("noise", a, b, "lanczos"))
    default = RZ.resize_on_device(images[:1], [picks[0][1]])
    assert np.array_equal(default[0].cpu().numpy(), RC.expected("noise", *picks[0], "bicubic"))
    for bad in (lambda: RZ.resize_on_device(images, [(20, 26)]), lambda: RZ.resize_on_device([images[0].float()], [(20, 26)]),
                lambda: RZ.resize_on_device(images[:1], [(4, 26)]), lambda: RZ.resize_on_device(images[:1], [(20, 26)], "box"),
                lambda: RZ.resize_on_device([torch.zeros(16, 16, 3, dtype=torch.uint8)], [(1, 1)])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------- (b) the refusals, with real buffers
def test_every_error_returns_minus_one_with_a_message_and_writes_nothing():
    # invalid arguments only: every one is refused on the host before anything is launched
    lib = RZ.lib()
    sizes = [(40, 52, 20, 26), (5, 7, 3, 2)]
    host_tables, tab_offsets = RZ.build_tables(sizes, "bicubic")
    tables = torch.from_numpy(np.concatenate([host_tables, np.zeros(4, np.int32)])).cuda()
    src = torch.full((16384,), 77, dtype=torch.uint8, device="cuda")
    dst = torch.full((16384,), SENTINEL, dtype=torch.uint8, device="cuda")
    scratch = torch.full((16384,), SENTINEL, dtype=torch.uint8, device="cuda")

    def rec(i=0, **kw):
        h_in, w_in, h_out, w_out = sizes[i]
        base = dict(src_off=8192 * i, dst_off=4096 * i, tab_off=tab_offsets[i], h_in=h_in, w_in=w_in, h_out=h_out, w_out=w_out)
        return RZ.ResizeImage(**dict(base, **kw))

    def call(images=None, n=None, **kw):
        images = [rec(0), rec(1)] if images is None else images
        a = dict(dict(src=src.data_ptr(), dst=dst.data_ptr(), filter=3, tables=tables.data_ptr(), tables_bytes=4 * tables.numel(),
                      scratch=scratch.data_ptr(), scratch_bytes=scratch.numel()), **kw)
        arr = (RZ.ResizeImage * len(images))(*images) if images != "null" else None
        rc = lib.srgd_resize_u8_images(a["src"], a["dst"], arr, len(images) if n is None else n, a["filter"], a["tables"],
                                       a["tables_bytes"], a["scratch"], a["scratch_bytes"],
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, lib.srgd_resize_last_error().decode()
    in_size, out_size = RC.REFUSED_CASES[0]
    cases = {"null": [dict(src=None), dict(dst=None), dict(tables=None), dict(scratch=None), dict(images="null", n=2)],
             "n_images": [dict(n=0)],
             "bad size": [dict(images=[rec(0), rec(1, h_in=0)]), dict(images=[rec(0, w_out=16385), rec(1)])],
             "ratio": [dict(images=[rec(0), rec(1, h_out=41)]), dict(images=[rec(0, w_in=3), rec(1)]),
                       dict(images=[rec(0), rec(1, h_in=in_size[0], w_in=in_size[1], h_out=out_size[0], w_out=out_size[1])])],
             "multiple of 16": [dict(images=[rec(0), rec(1, dst_off=4100)]), dict(images=[rec(0, src_off=8), rec(1)]),
                                dict(images=[rec(0), rec(1, tab_off=tab_offsets[1] + 4)])],
             "outside [0, 2^36)": [dict(images=[rec(0), rec(1, dst_off=-16)]), dict(images=[rec(0, src_off=1 << 36), rec(1)])],
             "unknown filter": [dict(filter=0), dict(filter=5)],
             "scratch must be 16-byte aligned": [dict(scratch=scratch.data_ptr() + 4)],
             "tables must be 16-byte aligned": [dict(tables=tables.data_ptr() + 8)],
             "tables_bytes": [dict(tables_bytes=tab_offsets[1] + 100)],
             "scratch_bytes": [dict(scratch_bytes=3 * 40 * 26)],
             "overlap": [dict(dst=src.data_ptr()), dict(dst=src.data_ptr() + 8192)]}
    for phrase, calls in cases.items():
        for kw in calls:
            rc, msg = call(**kw)
            assert rc == -1 and phrase in msg, (phrase, kw, msg)
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all()) and bool((scratch == SENTINEL).all()) and bool((src == 77).all())
    rc, msg = call()                                                          # the same call with nothing wrong in it runs
    torch.cuda.synchronize()
    assert rc == 0, msg
    want = RC.resize_u8(np.full((40, 52, 3), 77, np.uint8), 20, 26, "bicubic")
    assert np.array_equal(dst[:3 * 20 * 26].cpu().numpy().reshape(20, 26, 3), want) and bool((dst[3 * 20 * 26:4096] == SENTINEL).all())
    with pytest.raises(ValueError, match="do not fit"):
        RZ.resize_flat(src, [0], dst, [0], [(40, 52, 20, 26), (5, 7, 3, 2)])


# ------------------------------------------------------------------------------------------- (c) the command line
def _lr(h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng([seed, h, w])
    base = np.stack([128 + 90 * np.sin(x / 5.0 + seed) * np.cos(y / 6.0), 100 + 4.0 * x - 2.5 * y, 140 + 60 * np.cos((x + y) / 4.0)], axis=2)
    return np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)


def test_cli_outscale(tmp_path):
    from srgd_amd.synth import synth_state_dict
    from tests.test_engine_gpu import _schema
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    indir = tmp_path / "in"
    indir.mkdir()
    Image.fromarray(_lr(22, 24, 1), "RGB").save(indir / "a.png")
    Image.fromarray(_lr(24, 22, 2), "RGB").save(indir / "b.png")

    def run(outdir, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(indir),
               "--output_dir", str(tmp_path / outdir), "--num_sample_steps", "2", "--test_label", "1", "--batch_size", "4", "--device_noise",
               "--seed", "71", "--lockstep_tiles", "8", "--consistency", *extra]
        return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)

    def files(outdir):
        return {n: open(tmp_path / outdir / n, "rb").read() for n in sorted(os.listdir(tmp_path / outdir))}
    plain = run("plain")
    assert plain.returncode == 0, plain.stderr[-3000:]
    half = run("half", "--outscale", "2", "--outscale_filter", "lanczos")
    assert half.returncode == 0, half.stderr[-3000:]
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "half")) == ["a_out.png", "b_out.png", "consistency.json"]
    for name, lr_hw in (("a_out.png", (22, 24)), ("b_out.png", (24, 22))):
        x4 = np.asarray(Image.open(tmp_path / "plain" / name).convert("RGB"))
        x2 = np.asarray(Image.open(tmp_path / "half" / name).convert("RGB"))
        assert x4.shape == (4 * lr_hw[0], 4 * lr_hw[1], 3) and x2.shape == (2 * lr_hw[0], 2 * lr_hw[1], 3)
        assert x4.min() < x4.max()
        assert np.array_equal(x2, RC.resize_u8(x4, 2 * lr_hw[0], 2 * lr_hw[1], "lanczos")), name
    # --consistency measures the x4 image, before the resize
    assert json.load(open(tmp_path / "plain" / "consistency.json")) == json.load(open(tmp_path / "half" / "consistency.json"))
    same = run("same", "--outscale", "4")
    assert same.returncode == 0, same.stderr[-3000:]
    assert files("same") == files("plain")                                    # byte for byte
    refused = run("refused", "--samples", "2", "--ensemble", "--outscale", "2")
    assert refused.returncode != 0 and "--ensemble" in refused.stderr and "engine ready" not in refused.stdout
    assert not os.path.exists(tmp_path / "refused")
