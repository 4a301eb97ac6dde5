"""srgd_amd.alpha on the MI355X: every plane, pack and bleed case of tests/alpha_cases.py against the numpy restatements as equality,
each destination inside a larger sentinel-filled buffer whose other bytes must not change and the scratch untouched beyond what the
header says a call may use; groups against solo calls; the 128-image boundary of a launch sequence; the list API; the refusals with
real buffers; and --alpha keep / --alpha_bleed on the command line.

Pillow is imported for reading and writing PNG files only: the comparison target is the restatement, which tests/test_alpha_cpu.py
pins against Pillow itself.  The command-line test samples a 22x24 RGBA, a 24x22 RGB and a 22x22 P+tRNS input: a side of 20 pixels is
refused by the tiling of the sampler itself (a reflect pad of 88 rows on the 80 rows of its x4 image, as upstream), with or without
--alpha, so 22 is the smallest side that can be sampled."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import alpha as AL
from srgd_amd import resize as RZ
from tests import alpha_cases as AC
from tests import resize_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
GUARD = 64


def _round(n):
    return (n + 15) // 16 * 16


def _layout(sizes, order=None, lead=48, gap=32):
    """Offsets (multiples of 16) of images of ``sizes`` bytes placed in ``order`` with ``lead`` bytes in front and at least ``gap``
    bytes between two -> (offsets in the order of ``sizes``, total bytes)."""
    order = list(range(len(sizes))) if order is None else order
    offsets, at = [0] * len(sizes), lead
    for i in order:
        offsets[i] = at
        at += _round(sizes[i]) + gap
    return offsets, at


def _upload(arrays, fill=0x3C):
    """The arrays, flattened, 16 spare bytes apart in one device buffer -> (buffer, offsets)."""
    offsets, at = _layout([a.size for a in arrays], lead=0, gap=16)
    host = np.full(max(at, 16), fill, np.uint8)
    for a, off in zip(arrays, offsets):
        host[off:off + a.size] = a.reshape(-1)
    return torch.from_numpy(host).cuda(), offsets


def _finish(dst, dst_offsets, shapes, scratch, used):
    """-> (results, whether every byte outside the destinations and every scratch byte beyond ``used`` still holds the sentinel)."""
    torch.cuda.synchronize()
    whole = dst.cpu().numpy()
    inside = np.zeros(whole.size, bool)
    results = []
    for shape, off in zip(shapes, dst_offsets):
        n = int(np.prod(shape))
        inside[off:off + n] = True
        results.append(whole[off:off + n].reshape(shape))
    clean = (~inside).sum() >= 80 and bool((whole[~inside] == SENTINEL).all()) and bool((scratch[used:] == SENTINEL).all())
    return results, clean


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _planes(items, filter, **place):
    """``srgd_alpha_resize_planes`` on ``items`` = ``[(uint8 [h,w] array, (h_out, w_out))]`` -> (results, clean)."""
    src, src_offsets = _upload([p for p, _ in items])
    dst_offsets, total = _layout([h * w for _, (h, w) in items], **place)
    dst = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = [p.shape + tuple(out) for p, out in items]
    host_tables, tab_offsets = RZ.build_tables(sizes, filter)
    tables = torch.from_numpy(np.concatenate([host_tables, np.zeros(4, np.int32)])).cuda()
    used = AL.plane_scratch_bytes(sizes)
    scratch = torch.full((used + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    recs = (AL.AlphaPlane * len(items))(*[AL.AlphaPlane(so, do, to, *size, RC.ksize(size[1], size[3], filter), RC.ksize(size[0], size[2], filter))
                                          for so, do, to, size in zip(src_offsets, dst_offsets, tab_offsets, sizes)])
    rc = AL.lib().srgd_alpha_resize_planes(src.data_ptr(), dst.data_ptr(), recs, len(items), tables.data_ptr(), 4 * tables.numel(),
                                           scratch.data_ptr(), used, _stream())
    assert rc == 0, AL.lib().srgd_alpha_last_error()
    return _finish(dst, dst_offsets, [out for _, out in items], scratch, used)


def _pack(items, **place):
    """``srgd_alpha_pack_rgba`` on ``items`` = ``[(uint8 [h,w,3], uint8 [h,w])]`` -> (results, clean)."""
    rgb, rgb_offsets = _upload([c for c, _ in items])
    alpha, a_offsets = _upload([a for _, a in items])
    dst_offsets, total = _layout([4 * a.size for _, a in items], **place)
    dst = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    recs = (AL.AlphaImage * len(items))(*[AL.AlphaImage(co, ao, do, *a.shape) for co, ao, do, (_, a) in zip(rgb_offsets, a_offsets, dst_offsets, items)])
    rc = AL.lib().srgd_alpha_pack_rgba(rgb.data_ptr(), alpha.data_ptr(), dst.data_ptr(), recs, len(items), _stream())
    assert rc == 0, AL.lib().srgd_alpha_last_error()
    return _finish(dst, dst_offsets, [a.shape + (4,) for _, a in items], torch.full((GUARD,), SENTINEL, dtype=torch.uint8), 0)


def _bleed(images, passes, **place):
    """``srgd_alpha_bleed`` on uint8 [h,w,4] arrays -> (results, clean)."""
    src, src_offsets = _upload(images)
    dst_offsets, total = _layout([3 * im.shape[0] * im.shape[1] for im in images], **place)
    dst = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    used = AL.bleed_scratch_bytes([im.shape[:2] for im in images]) if passes else 0
    scratch = torch.full((used + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    recs = (AL.AlphaImage * len(images))(*[AL.AlphaImage(do, 0, so, *im.shape[:2]) for so, do, im in zip(src_offsets, dst_offsets, images)])
    rc = AL.lib().srgd_alpha_bleed(src.data_ptr(), dst.data_ptr(), recs, len(images), passes, scratch.data_ptr(), used, _stream())
    assert rc == 0, AL.lib().srgd_alpha_last_error()
    return _finish(dst, dst_offsets, [im.shape[:2] + (3,) for im in images], scratch, used)


# ------------------------------------------------------------------------------------------- (a) the kernels are the restatements
@pytest.mark.parametrize("filter", list(RC.FILTERS))
def test_every_plane_case_is_the_restatement_bit_for_bit_and_nothing_else_is_written(filter):
    for in_size, out_size in AC.PLANE_CASES:
        for name in AC.PATTERNS:
            (got,), clean = _planes([(AC.plane(name, *in_size), out_size)], filter)
            want = AC.expected_plane(name, in_size, out_size, filter)
            assert got.shape == want.shape and np.array_equal(got, want), (in_size, out_size, filter, name, int((got != want).sum()))
            assert clean, (in_size, out_size, filter, name)


def test_every_pack_case_is_the_restatement_and_nothing_else_is_written():
    for h, w in AC.PACK_SIZES:
        (got,), clean = _pack([(AC.colour(h, w), AC.plane("noise", h, w))])
        assert np.array_equal(got, AC.pack(AC.colour(h, w), AC.plane("noise", h, w))) and clean, (h, w)


@pytest.mark.parametrize("passes", AC.BLEED_PASSES)
def test_every_bleed_case_is_the_restatement_and_nothing_else_is_written(passes):
    for h, w in AC.BLEED_SIZES:
        for name in AC.BLEED_PATTERNS:
            (got,), clean = _bleed([AC.bleed_image(name, h, w)], passes)
            want = AC.expected_bleed(name, h, w, passes)
            assert np.array_equal(got, want) and clean, (h, w, name, passes, int((got != want).sum()))


def test_every_image_of_a_group_is_its_solo_call():
    picks = [((129, 67), (43, 100)), ((33, 65), (33, 31)), ((8, 6), (64, 48)), ((17, 65), (17, 65)), ((16, 100), (17, 65))]
    assert all(case in AC.PLANE_CASES for case in picks)
    for filter in RC.FILTERS:
        items = [(AC.plane("noise", *a), b) for a, b in picks]
        grouped, clean = _planes(items, filter, order=[2, 0, 4, 3, 1], lead=16, gap=80)
        assert clean
        for item, (a, b), got in zip(items, picks, grouped):
            (solo,), _ = _planes([item], filter, lead=0)
            assert np.array_equal(got, solo) and np.array_equal(got, AC.expected_plane("noise", a, b, filter)), (a, b, filter)
    items = [(AC.colour(h, w), AC.plane("checker", h, w)) for h, w in AC.PACK_SIZES]
    order = list(reversed(range(len(items))))
    grouped, clean = _pack(items, order=order, lead=16, gap=80)
    assert clean
    for item, got in zip(items, grouped):
        (solo,), _ = _pack([item], lead=0)
        assert np.array_equal(got, solo) and np.array_equal(got, AC.pack(*item))
    images = [AC.bleed_image(name, h, w) for (h, w), name in zip(AC.BLEED_SIZES + AC.BLEED_SIZES[::-1], AC.BLEED_PATTERNS + ("random70", "corner", "one_254"))]
    for passes in (0, 1, 5):
        grouped, clean = _bleed(images, passes, order=[3, 1, 0, 2, 7, 6, 5, 4], lead=16, gap=80)
        assert clean
        for im, got in zip(images, grouped):
            (solo,), _ = _bleed([im], passes, lead=0)
            assert np.array_equal(got, solo) and np.array_equal(got, AC.bleed(im, passes)), (im.shape, passes)


def test_a_group_of_130_crosses_the_launch_sequence_boundary():
    rng = np.random.default_rng(7)
    check = (0, 1, 63, 127, 128, 129)                                         # solo calls on both sides of the boundary
    planes = [rng.integers(0, 256, (5, 7), dtype=np.uint8) for _ in range(130)]
    grouped, clean = _planes([(p, (3, 9)) for p in planes], "bicubic")
    assert clean
    for i, (p, got) in enumerate(zip(planes, grouped)):
        if i in check:
            (solo,), _ = _planes([(p, (3, 9))], "bicubic")
            assert np.array_equal(got, solo), i
        assert np.array_equal(got, AC.resize_plane(p, 3, 9, "bicubic")), i
    items = [(rng.integers(0, 256, (3, 3 + i % 3, 3), dtype=np.uint8), rng.integers(0, 256, (3, 3 + i % 3), dtype=np.uint8)) for i in range(130)]
    grouped, clean = _pack(items)
    assert clean and all(np.array_equal(got, AC.pack(*item)) for item, got in zip(items, grouped))
    images = [np.dstack([rng.integers(0, 256, (4, 5 + i % 2, 3), dtype=np.uint8), np.where(rng.random((4, 5 + i % 2)) < 0.8, 0, 9).astype(np.uint8)])
              for i in range(130)]
    grouped, clean = _bleed(images, 2)
    assert clean
    for i, (im, got) in enumerate(zip(images, grouped)):
        if i in check:
            (solo,), _ = _bleed([im], 2)
            assert np.array_equal(got, solo), i
        assert np.array_equal(got, AC.bleed(im, 2)), i


def test_the_list_apis_move_images_to_the_gpu_and_return_device_tensors():
    picks = [((40, 52), (20, 26)), ((40, 52), (30, 39)), ((37, 23), (23, 37))]
    planes = [torch.from_numpy(AC.plane("noise", *a).copy()) for a, _ in picks]
    planes[1] = planes[1].cuda()
    outs = AL.resize_planes_on_device(planes, [b for _, b in picks], "lanczos")
    for (a, b), out in zip(picks, outs):
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == b
        assert np.array_equal(out.cpu().numpy(), AC.expected_plane("noise", a, b, "lanczos"))
    default = AL.resize_planes_on_device(planes[:1], [picks[0][1]])
    assert np.array_equal(default[0].cpu().numpy(), AC.expected_plane("noise", *picks[0], "bicubic"))
    images = [torch.from_numpy(AC.bleed_image("random70", h, w).copy()) for h, w in AC.BLEED_SIZES]
    images[2] = images[2].cuda()
    for passes in (0, 3):
        for (h, w), out in zip(AC.BLEED_SIZES, AL.bleed_on_device(images, passes)):
            assert out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), AC.expected_bleed("random70", h, w, passes) if passes == 0
                                                                                  else AC.bleed(AC.bleed_image("random70", h, w), passes))
    # attach: x4 alone, the two-stage path down and up, a 1x1 input; host and device tensors mixed
    cases = [((10, 13), (40, 52)), ((10, 13), (20, 26)), ((10, 13), (30, 39)), ((1, 1), (4, 4)), ((5, 7), (3, 4)), ((3, 5), (96, 160))]
    for filter in RC.FILTERS:
        rgbs = [torch.from_numpy(AC.colour(*final).copy()) for _, final in cases]
        lows = [torch.from_numpy(AC.plane("noise", *lr).copy()) for lr, _ in cases]
        rgbs[0], lows[1] = rgbs[0].cuda(), lows[1].cuda()
        for (lr, final), out in zip(cases, AL.attach_alpha_on_device(rgbs, lows, 4, filter)):
            assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == final + (4,)
            assert np.array_equal(out.cpu().numpy(), AC.attach(AC.colour(*final), AC.plane("noise", *lr), 4, filter)), (lr, final, filter)
    for bad in (lambda: AL.resize_planes_on_device(planes, [(20, 26)]), lambda: AL.resize_planes_on_device([planes[0].float()], [(20, 26)]),
                lambda: AL.resize_planes_on_device(planes[:1], [(4, 26)]), lambda: AL.bleed_on_device(images, 65),
                lambda: AL.attach_alpha_on_device([rgbs[0]], [lows[0]], 4, "box")):
        with pytest.raises(ValueError):
            bad()


# both tilings' edges (32- and 64-pixel horizontal tiles, 16-row tiles), the dword and the byte paths, the 49-tap table, one-pass forms
PLANE_IS_CHANNEL_GEOMETRIES = [((5, 7), (3, 2)), ((17, 70), (33, 131)), ((16, 64), (64, 256)), ((40, 52), (20, 26)), ((64, 264), (8, 33)),
                               ((9, 12), (9, 24)), ((12, 9), (24, 9))]


@pytest.mark.parametrize("filter", list(RC.FILTERS))
def test_a_plane_is_a_channel_of_the_rgb_resize(filter):
    # the two libraries instantiate one template (pillow_resample.hpp): <3 channels, 32 pixels, 2 rows> and <1, 64, 4>
    g = torch.Generator().manual_seed(20)
    images = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for (h, w), _ in PLANE_IS_CHANNEL_GEOMETRIES]
    sizes = [out for _, out in PLANE_IS_CHANNEL_GEOMETRIES]
    rgb = RZ.resize_on_device(images, sizes, filter)
    planes = AL.resize_planes_on_device([im[:, :, c].contiguous() for im in images for c in range(3)], [s for s in sizes for _ in range(3)], filter)
    for i, (geometry, out) in enumerate(zip(PLANE_IS_CHANNEL_GEOMETRIES, rgb)):
        assert tuple(out.shape) == geometry[1] + (3,)
        for c in range(3):
            assert torch.equal(planes[3 * i + c], out[:, :, c]), (geometry, filter, c)


# ------------------------------------------------------------------------------------------- (b) the refusals, with real buffers
def test_every_error_returns_minus_one_with_a_message_and_writes_nothing():
    # invalid arguments only: every one is refused on the host before anything is launched
    lib = AL.lib()
    sizes = [(40, 52, 20, 26), (5, 7, 3, 2)]
    host_tables, tab_offsets = RZ.build_tables(sizes, "bicubic")
    tables = torch.from_numpy(np.concatenate([host_tables, np.zeros(4, np.int32)])).cuda()
    src = torch.full((16384,), 77, dtype=torch.uint8, device="cuda")
    other = torch.full((16384,), 78, dtype=torch.uint8, device="cuda")
    dst = torch.full((16384,), SENTINEL, dtype=torch.uint8, device="cuda")
    scratch = torch.full((16384,), SENTINEL, dtype=torch.uint8, device="cuda")

    def plane(i=0, **kw):
        h_in, w_in, h_out, w_out = sizes[i]
        base = dict(src_off=8192 * i, dst_off=4096 * i, tab_off=tab_offsets[i], h_in=h_in, w_in=w_in, h_out=h_out, w_out=w_out,
                    k_h=RC.ksize(w_in, w_out, "bicubic"), k_v=RC.ksize(h_in, h_out, "bicubic"))
        return AL.AlphaPlane(**dict(base, **kw))

    def resize(planes=None, n=None, **kw):
        planes = [plane(0), plane(1)] if planes is None else planes
        a = dict(dict(src=src.data_ptr(), dst=dst.data_ptr(), tables=tables.data_ptr(), tables_bytes=4 * tables.numel(),
                      scratch=scratch.data_ptr(), scratch_bytes=scratch.numel()), **kw)
        rc = lib.srgd_alpha_resize_planes(a["src"], a["dst"], (AL.AlphaPlane * len(planes))(*planes), len(planes) if n is None else n,
                                          a["tables"], a["tables_bytes"], a["scratch"], a["scratch_bytes"], _stream())
        return rc, lib.srgd_alpha_last_error().decode()

    def image(i=0, **kw):
        return AL.AlphaImage(**dict(dict(rgb_off=4096 * i, a_off=8192 * i, rgba_off=4096 * i, h=7 - i, w=5 + i), **kw))

    def pack(images=None, n=None, **kw):
        images = [image(0), image(1)] if images is None else images
        a = dict(dict(rgb=src.data_ptr(), alpha=other.data_ptr(), rgba=dst.data_ptr()), **kw)
        rc = lib.srgd_alpha_pack_rgba(a["rgb"], a["alpha"], a["rgba"], (AL.AlphaImage * len(images))(*images), len(images) if n is None else n, _stream())
        return rc, lib.srgd_alpha_last_error().decode()

    def bleed(images=None, n=None, **kw):
        images = [image(0), image(1)] if images is None else images
        a = dict(dict(rgba=src.data_ptr(), rgb=dst.data_ptr(), passes=3, scratch=scratch.data_ptr(), scratch_bytes=scratch.numel()), **kw)
        rc = lib.srgd_alpha_bleed(a["rgba"], a["rgb"], (AL.AlphaImage * len(images))(*images), len(images) if n is None else n, a["passes"],
                                  a["scratch"], a["scratch_bytes"], _stream())
        return rc, lib.srgd_alpha_last_error().decode()
    in_size, out_size = RC.REFUSED_CASES[0]
    every = [(resize, {"null": [dict(src=None), dict(dst=None), dict(tables=None), dict(scratch=None)],
                       "n_planes": [dict(n=0)],
                       "bad size": [dict(planes=[plane(0), plane(1, h_in=0)]), dict(planes=[plane(0, w_out=16385), plane(1)])],
                       "ratio": [dict(planes=[plane(0), plane(1, h_out=41)]), dict(planes=[plane(0, w_in=3), plane(1)]),
                                 dict(planes=[plane(0), plane(1, h_in=in_size[0], w_in=in_size[1], h_out=out_size[0], w_out=out_size[1])])],
                       "ksize": [dict(planes=[plane(0), plane(1, k_h=0)]), dict(planes=[plane(0, k_v=50), plane(1)])],
                       "multiple of 16": [dict(planes=[plane(0), plane(1, dst_off=4100)]), dict(planes=[plane(0, src_off=8), plane(1)]),
                                          dict(planes=[plane(0), plane(1, tab_off=tab_offsets[1] + 4)])],
                       "outside [0, 2^36)": [dict(planes=[plane(0), plane(1, dst_off=-16)]), dict(planes=[plane(0, src_off=1 << 36), plane(1)])],
                       "16-byte aligned": [dict(scratch=scratch.data_ptr() + 4), dict(tables=tables.data_ptr() + 8), dict(dst=dst.data_ptr() + 4)],
                       "tables_bytes": [dict(tables_bytes=tab_offsets[1] + 100)],
                       "scratch_bytes": [dict(scratch_bytes=40 * 26)],
                       "overlap": [dict(dst=src.data_ptr()), dict(dst=src.data_ptr() + 8192)]}),
             (pack, {"null": [dict(rgb=None), dict(alpha=None), dict(rgba=None)], "n_images": [dict(n=0)],
                     "bad size": [dict(images=[image(0), image(1, h=0)]), dict(images=[image(0, w=16385), image(1)])],
                     "multiple of 16": [dict(images=[image(0), image(1, rgba_off=4100)]), dict(images=[image(0, a_off=8), image(1)])],
                     "outside [0, 2^36)": [dict(images=[image(0), image(1, rgb_off=-16)])],
                     "16-byte aligned": [dict(rgba=dst.data_ptr() + 8)],
                     "overlap": [dict(rgba=src.data_ptr()), dict(rgba=other.data_ptr() + 8192)]}),
             (bleed, {"null": [dict(rgba=None), dict(rgb=None), dict(scratch=None)], "n_images": [dict(n=0)], "passes": [dict(passes=65), dict(passes=-1)],
                      "bad size": [dict(images=[image(0), image(1, w=0)])],
                      "multiple of 16": [dict(images=[image(0), image(1, rgb_off=4100)])],
                      "outside [0, 2^36)": [dict(images=[image(0, rgba_off=1 << 36), image(1)])],
                      "16-byte aligned": [dict(scratch=scratch.data_ptr() + 4), dict(rgb=dst.data_ptr() + 4)],
                      "scratch_bytes": [dict(scratch_bytes=2 * (144 + 144) - 16)],
                      "overlap": [dict(rgb=src.data_ptr()), dict(rgb=src.data_ptr() + 4096)]})]
    for call, cases in every:
        for phrase, calls in cases.items():
            for kw in calls:
                rc, msg = call(**kw)
                assert rc == -1 and phrase in msg, (call.__name__, phrase, kw, msg)
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all()) and bool((scratch == SENTINEL).all()) and bool((src == 77).all()) and bool((other == 78).all())
    rc, msg = resize()                                                        # the same calls with nothing wrong in them run
    torch.cuda.synchronize()
    assert rc == 0, msg
    want = AC.resize_plane(np.full((40, 52), 77, np.uint8), 20, 26, "bicubic")
    assert np.array_equal(dst[:20 * 26].cpu().numpy().reshape(20, 26), want) and bool((dst[20 * 26:4096] == SENTINEL).all())
    dst.fill_(SENTINEL)
    rc, msg = pack()
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert dst[:4 * 35].cpu().numpy().reshape(35, 4).tolist() == [[77, 77, 77, 78]] * 35 and bool((dst[4 * 35:4096] == SENTINEL).all())
    dst.fill_(SENTINEL)
    rc, msg = bleed()
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert bool((dst[:3 * 35] == 77).all()) and bool((dst[3 * 35:4096] == SENTINEL).all())
    with pytest.raises(ValueError, match="do not fit"):
        AL.resize_planes_flat(src, [0], dst, [0], [(40, 52, 20, 26), (5, 7, 3, 2)])
    with pytest.raises(ValueError, match="do not fit"):
        AL.bleed_flat(src, [0, 16368], dst, [0, 4096], [(7, 5), (6, 6)], 2)


# ------------------------------------------------------------------------------------------- (c) the command line
def _lr(h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng([seed, h, w])
    base = np.stack([128 + 90 * np.sin(x / 5.0 + seed) * np.cos(y / 6.0), 100 + 4.0 * x - 2.5 * y, 140 + 60 * np.cos((x + y) / 4.0)], axis=2)
    return np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)


def test_cli_alpha(tmp_path):
    """Four model runs and one refusal.  The issue asked for a 20x20 P+tRNS input; the sampler's tiling refuses any side of 20 pixels
    (with or without this feature), so c.png is 22x22, the smallest size that can be sampled - nothing else about the case changes."""
    from srgd_amd.synth import synth_state_dict
    from tests.test_engine_gpu import _schema
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    rng = np.random.default_rng(17)
    indir, bled_dir = tmp_path / "in", tmp_path / "in_bled"
    indir.mkdir()
    bled_dir.mkdir()
    # a.png: RGBA, about half of the alpha zero in blobs, black stored under the transparent pixels (what makes the halo)
    yy, xx = np.mgrid[0:22, 0:24]
    a_alpha = np.where(np.sin(yy / 2.5) + np.cos(xx / 3.0) > 0.1, rng.integers(1, 256, (22, 24)), 0).astype(np.uint8)
    assert 0.35 < (a_alpha == 0).mean() < 0.65
    a_rgb = np.where(a_alpha[:, :, None] > 0, _lr(22, 24, 1), 0).astype(np.uint8)
    Image.fromarray(np.dstack([a_rgb, a_alpha]), "RGBA").save(indir / "a.png")
    b_rgb = _lr(24, 22, 2)
    Image.fromarray(b_rgb, "RGB").save(indir / "b.png")
    # c.png: a 6-colour palette with a tRNS chunk: two entries fully transparent, one half
    c_idx = ((yy[:, :22] // 3 + xx[:22, :22] // 4) % 6).astype(np.uint8)
    pal = Image.fromarray(c_idx, "P")
    pal.putpalette([0, 0, 0, 220, 40, 40, 40, 200, 60, 30, 60, 230, 240, 240, 20, 250, 250, 250] + [0] * (3 * 250))
    pal.save(indir / "c.png", transparency=bytes([0, 255, 255, 128, 0, 255]))
    with Image.open(indir / "c.png") as im:
        assert im.mode == "P" and im.has_transparency_data
        c_rgb, c_alpha = np.asarray(im.convert("RGB")), AL.alpha_of(im)
    assert c_alpha.shape == (22, 22) and set(np.unique(c_alpha)) == {0, 128, 255}
    lows = {"a_out.png": (a_rgb, a_alpha), "b_out.png": (b_rgb, None), "c_out.png": (c_rgb, c_alpha)}
    for name, (rgb, plane) in lows.items():                                   # run 4 reads the restatement's bled images as plain RGB
        bled = rgb if plane is None else AC.bleed(np.dstack([rgb, plane]), 3)
        Image.fromarray(bled, "RGB").save(bled_dir / name.replace("_out", ""))
    assert not np.array_equal(AC.bleed(np.dstack([a_rgb, a_alpha]), 3), a_rgb)

    def run(outdir, *extra, source=indir):
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(source),
               "--output_dir", str(tmp_path / outdir), "--num_sample_steps", "2", "--test_label", "1", "--batch_size", "4", "--device_noise",
               "--seed", "71", "--lockstep_tiles", "8", "--consistency", *extra]
        return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)

    def files(outdir):
        return {n: open(tmp_path / outdir / n, "rb").read() for n in sorted(os.listdir(tmp_path / outdir))}

    def load(outdir, name):
        with Image.open(tmp_path / outdir / name) as im:
            return im.mode, np.asarray(im)
    names = ["a_out.png", "b_out.png", "c_out.png", "consistency.json"]
    outscale = ("--outscale", "2", "--outscale_filter", "lanczos")
    plain = run("plain")                                                      # 1
    assert plain.returncode == 0, plain.stderr[-3000:]
    keep = run("keep", "--alpha", "keep")                                     # 2
    assert keep.returncode == 0, keep.stderr[-3000:]
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "keep")) == names
    for name in ("a_out.png", "c_out.png"):
        rgb, plane = lows[name]
        mode1, x1 = load("plain", name)
        mode2, x2 = load("keep", name)
        assert mode1 == "RGB" and mode2 == "RGBA" and x2.shape == (4 * plane.shape[0], 4 * plane.shape[1], 4) and x1.min() < x1.max()
        assert np.array_equal(x2[:, :, :3], x1), name                         # the colour of a run without the flag
        assert np.array_equal(x2, AC.attach(x1, plane, 4, "bicubic")), name
    assert files("keep")["b_out.png"] == files("plain")["b_out.png"] and files("keep")["consistency.json"] == files("plain")["consistency.json"]
    bled = run("bled", "--alpha", "keep", "--alpha_bleed", "3", *outscale)   # 3
    assert bled.returncode == 0, bled.stderr[-3000:]
    ref = run("ref", *outscale, source=bled_dir)                              # 4
    assert ref.returncode == 0, ref.stderr[-3000:]
    assert sorted(os.listdir(tmp_path / "bled")) == sorted(os.listdir(tmp_path / "ref")) == names
    assert json.load(open(tmp_path / "bled" / "consistency.json")) == json.load(open(tmp_path / "ref" / "consistency.json"))
    assert files("bled")["b_out.png"] == files("ref")["b_out.png"]
    for name in ("a_out.png", "c_out.png"):
        rgb, plane = lows[name]
        mode3, x3 = load("bled", name)
        mode4, x4 = load("ref", name)
        h, w = plane.shape
        assert mode3 == "RGBA" and mode4 == "RGB" and x3.shape == (2 * h, 2 * w, 4)
        assert np.array_equal(x3[:, :, :3], x4), name                         # the model was given the restatement's bled image
        assert np.array_equal(x3, AC.attach(x4, plane, 4, "lanczos")), name   # the two-stage alpha: x4 bicubic, then lanczos to x2
    _, a1 = load("plain", "a_out.png")
    assert not np.array_equal(load("bled", "a_out.png")[1][:, :, :3], RC.resize_u8(a1, 44, 48, "lanczos"))       # the bleed reached the model
    refused = run("refused", "--alpha", "keep", "--samples", "2", "--ensemble")  # 5
    assert refused.returncode != 0 and "--ensemble" in refused.stderr and "engine ready" not in refused.stdout
    assert not os.path.exists(tmp_path / "refused")
