"""srgd_amd.selfens on the MI355X: every size x op of tests/selfens_cases.py through srgd_selfens_transform and every size x source
list through srgd_selfens_merge against the numpy restatement as equality (mean01 as exact fp32 equality), each destination inside a
larger sentinel-filled buffer whose other bytes must not change, sources at offsets that are multiples of 16 but not of 32 with other
data around them; groups against solo calls; the 32-image boundary of a launch; the list APIs; the refusals with real buffers; and
--self_ensemble on the command line against plain runs over the numpy-transformed inputs.

Pillow is imported for reading and writing PNG files only: the comparison target is the restatement, which tests/test_selfens_cpu.py
pins against the definition."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import _lib
from srgd_amd import consistency as CS
from srgd_amd import metrics as MX
from srgd_amd import selfens as SE
from tests import selfens_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
MERGE_LISTS = list(SC.OP_LISTS.values()) + [SC.REPEATED]


def _round(n, to=16):
    return (n + to - 1) // to * to


def _upload(arrays, fill=0x3C):
    """The arrays, flattened, in one device buffer filled with other data, each at an offset that is a multiple of 16 but not of 32
    -> (buffer, offsets)."""
    offsets, at = [], 16
    for a in arrays:
        offsets.append(at)
        at += _round(a.size, 32) + 32
    assert all(off % 32 == 16 for off in offsets)
    host = np.full(at, fill, np.uint8)
    for a, off in zip(arrays, offsets):
        host[off:off + a.size] = a.reshape(-1)
    return torch.from_numpy(host).cuda(), offsets


def _layout(sizes, order=None, lead=48, gap=32):
    """Offsets (multiples of 16) of images of ``sizes`` bytes placed in ``order`` with ``lead`` bytes in front and at least ``gap``
    bytes between two -> (offsets in the order of ``sizes``, total bytes)."""
    order = list(range(len(sizes))) if order is None else order
    offsets, at = [0] * len(sizes), lead
    for i in order:
        offsets[i] = at
        at += _round(sizes[i]) + gap
    return offsets, at


def _finish(dst, dst_offsets, shapes):
    """-> (results, whether every byte outside the destinations still holds the sentinel; at least 80 of them)."""
    torch.cuda.synchronize()
    whole = dst.cpu().numpy()
    inside = np.zeros(whole.size, bool)
    results = []
    for shape, off in zip(shapes, dst_offsets):
        n = int(np.prod(shape))
        inside[off:off + n] = True
        results.append(whole[off:off + n].reshape(shape).copy())
    return results, bool((~inside).sum() >= 80 and (whole[~inside] == SENTINEL).all())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _transform(items, **place):
    """``srgd_selfens_transform`` on ``items`` = ``[(uint8 [h,w,3] array, op)]`` -> (results, clean)."""
    src, src_offsets = _upload([x for x, _ in items])
    dst_offsets, total = _layout([x.size for x, _ in items], **place)
    dst = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    recs = (SE.SelfensRecord * len(items))(*[SE.SelfensRecord(so, do, x.shape[0], x.shape[1], op, 0)
                                             for so, do, (x, op) in zip(src_offsets, dst_offsets, items)])
    rc = SE.lib().srgd_selfens_transform(src.data_ptr(), dst.data_ptr(), recs, len(items), _stream())
    assert rc == 0, SE.lib().srgd_selfens_last_error()
    return _finish(dst, dst_offsets, [SE.out_size(x.shape[0], x.shape[1], op) + (3,) for x, op in items])


def _merge(items, mean01=True, **place):
    """``srgd_selfens_merge`` on ``items`` = ``[(sources, ops)]`` -> (merged images, mean01 planes or None, clean)."""
    flat = [s for sources, _ in items for s in sources]
    src, flat_offsets = _upload(flat)
    shapes = [SE.out_size(sources[0].shape[0], sources[0].shape[1], SE.inverse(ops[0])) + (3,) for sources, ops in items]
    nbytes = [int(np.prod(s)) for s in shapes]
    dst_offsets, total = _layout(nbytes, **place)
    dst = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    m_offsets, m_total = [], 5                                                # unaligned, with guard floats around
    for n in nbytes:
        m_offsets.append(m_total)
        m_total += n + 23
    m01 = torch.full((m_total,), float("nan"), dtype=torch.float32, device="cuda") if mean01 else None
    images = (SE.SelfensImage * len(items))()
    at = 0
    for i, (sources, ops) in enumerate(items):
        images[i].dst_off, images[i].mean01_off = dst_offsets[i], m_offsets[i]
        images[i].H, images[i].W, images[i].n_src = shapes[i][0], shapes[i][1], len(sources)
        for j, op in enumerate(ops):
            images[i].src_off[j], images[i].op[j] = flat_offsets[at + j], op
        at += len(sources)
    rc = SE.lib().srgd_selfens_merge(src.data_ptr(), dst.data_ptr(), m01.data_ptr() if mean01 else None, images, len(items), _stream())
    assert rc == 0, SE.lib().srgd_selfens_last_error()
    results, clean = _finish(dst, dst_offsets, shapes)
    planes = None
    if mean01:
        whole = m01.cpu().numpy()
        inside = np.zeros(whole.size, bool)
        planes = []
        for (h, w, _), off, n in zip(shapes, m_offsets, nbytes):
            inside[off:off + n] = True
            planes.append(whole[off:off + n].reshape(3, h, w).copy())
        clean = clean and bool(np.isnan(whole[~inside]).all()) and (~inside).sum() >= 28
    return results, planes, clean


def _same_floats(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------- (a) the kernels are the restatements
@pytest.mark.parametrize("size", SC.SIZES)
def test_every_size_and_op_is_the_restatement_and_nothing_else_is_written(size):
    x = SC.image(*size)
    for op in range(8):
        (got,), clean = _transform([(x, op)])
        want = SC.apply(x, op)
        assert got.shape == want.shape and np.array_equal(got, want), (size, op, int((got != want).sum()))
        assert clean, (size, op)


@pytest.mark.parametrize("size", SC.SIZES)
def test_every_size_and_source_list_is_the_restatement_and_nothing_else_is_written(size):
    h, w = size
    for ops in MERGE_LISTS:
        sources = SC.sources(h, w, ops, "random", seed=len(ops))
        (got,), (planes,), clean = _merge([(sources, ops)])
        want = SC.merge(sources, ops)
        assert got.shape == want.shape and np.array_equal(got, want), (size, ops, int((got != want).sum()))
        assert _same_floats(planes, SC.mean01(want)), (size, ops)
        assert clean, (size, ops)
    for n in (2, 4, 8):                                                        # halves up, and the width of the sums
        sources = SC.sources(h, w, SC.OPS[n], "halves")
        (got,), _, clean = _merge([(sources, SC.OPS[n])], mean01=False)
        assert np.array_equal(got, SC.halves_expected(h, w, n)) and np.array_equal(got, SC.merge(sources, SC.OPS[n])) and clean, (size, n)
    (got,), (planes,), clean = _merge([(SC.sources(h, w, SC.OPS[8], "ones"), SC.OPS[8])])
    assert (got == 255).all() and (planes == np.float32(1.0)).all() and clean, size


def test_every_image_of_a_group_is_its_solo_call():
    items = [(SC.image(h, w, seed=i), (3 * i + 5) % 8) for i, (h, w) in enumerate(SC.SIZES)]
    order = [4, 0, 9, 2, 7, 1, 8, 3, 6, 5]
    grouped, clean = _transform(items, order=order, lead=16, gap=80)
    assert clean
    for (x, op), got in zip(items, grouped):
        (solo,), _ = _transform([(x, op)], lead=0)
        assert np.array_equal(got, solo) and np.array_equal(got, SC.apply(x, op)), (x.shape, op)
    items = [(SC.sources(h, w, MERGE_LISTS[i % len(MERGE_LISTS)], "random", seed=i), MERGE_LISTS[i % len(MERGE_LISTS)]) for i, (h, w) in enumerate(SC.SIZES)]
    grouped, planes, clean = _merge(items, order=order, lead=16, gap=80)
    assert clean
    for (sources, ops), got, pl in zip(items, grouped, planes):
        (solo,), (solo_planes,), _ = _merge([(sources, ops)], lead=0)
        want = SC.merge(sources, ops)
        assert np.array_equal(got, solo) and np.array_equal(got, want) and _same_floats(pl, solo_planes) and _same_floats(pl, SC.mean01(want)), ops


def test_a_group_of_33_crosses_the_launch_boundary():
    assert SE.MAX_IMAGES == SC.MAX_IMAGES == 32
    rng = np.random.default_rng(7)
    check = (0, 1, 31, 32)                                                     # solo calls on both sides of the boundary
    items = [(rng.integers(0, 256, (3 + i % 3, 5 + i % 4, 3), dtype=np.uint8), i % 8) for i in range(33)]
    grouped, clean = _transform(items)
    assert clean
    for i, ((x, op), got) in enumerate(zip(items, grouped)):
        if i in check:
            (solo,), _ = _transform([(x, op)])
            assert np.array_equal(got, solo), i
        assert np.array_equal(got, SC.apply(x, op)), i
    items = [(SC.sources(4 + i % 2, 33 + i % 3, MERGE_LISTS[i % len(MERGE_LISTS)], "random", seed=i), MERGE_LISTS[i % len(MERGE_LISTS)]) for i in range(33)]
    grouped, planes, clean = _merge(items)
    assert clean
    for i, ((sources, ops), got, pl) in enumerate(zip(items, grouped, planes)):
        if i in check:
            (solo,), (solo_planes,), _ = _merge([(sources, ops)])
            assert np.array_equal(got, solo) and _same_floats(pl, solo_planes), i
        assert np.array_equal(got, SC.merge(sources, ops)) and _same_floats(pl, SC.mean01(SC.merge(sources, ops))), i


def test_the_list_apis_return_device_tensors_equal_to_the_restatement():
    xs = [SC.image(h, w, seed=9) for h, w in ((5, 6), (63, 65), (16, 341))]
    tensors = [torch.from_numpy(x).cuda() for x in xs]
    ops = [5, 6, 3]
    outs = SE.dihedral_on_device(tensors, ops)
    for x, op, out in zip(xs, ops, outs):
        assert out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), SC.apply(x, op))
    eight = SE.dihedral_on_device([tensors[1]] * 8, list(range(8)))            # what the driver asks for: one image, every op
    assert all(np.array_equal(t.cpu().numpy(), SC.apply(xs[1], op)) for op, t in enumerate(eight))
    groups, wants = [], []
    for i, ((h, w), ops) in enumerate((((5, 6), SC.OPS[8]), ((63, 65), SC.OP_LISTS[3]), ((16, 341), SC.OPS[2]), ((7, 1), SC.REPEATED))):
        sources = SC.sources(h, w, ops, "random", seed=20 + i)
        groups.append([(torch.from_numpy(s).cuda(), op) for s, op in zip(sources, ops)])
        wants.append(SC.merge(sources, ops))
    for got, want in zip(SE.self_ensemble_on_device(groups), wants):
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    for (got, m01), want in zip(SE.self_ensemble_on_device(groups, return_mean01=True), wants):
        assert np.array_equal(got.cpu().numpy(), want) and m01.is_cuda and tuple(m01.shape) == (1, 3) + want.shape[:2]
        assert _same_floats(m01[0].cpu().numpy(), SC.mean01(want))
    # the merge of the turned outputs of the identity "model" is the image itself
    back = SE.self_ensemble_on_device([[(t, op) for op, t in enumerate(eight)]])[0]
    assert np.array_equal(back.cpu().numpy(), xs[1])
    for bad in (lambda: SE.dihedral_on_device(tensors, [0]), lambda: SE.dihedral_on_device([tensors[0].float()], [0]),
                lambda: SE.self_ensemble_on_device([[(tensors[0], 0), (tensors[0], 4)]]), lambda: SE.self_ensemble_on_device([[(tensors[0], 9)]])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.SrgdHipError):
        SE.dihedral_on_device([tensors[0].cpu()], [1])
    with pytest.raises(_lib.SrgdHipError):
        SE.self_ensemble_on_device([[(tensors[0], 0), (tensors[0].cpu(), 0)]])


# ------------------------------------------------------------------------------------------- (b) the refusals, with real buffers
def test_every_error_returns_minus_one_with_a_message_and_writes_nothing():
    # invalid arguments only: every one is refused on the host before anything is launched
    lib = SE.lib()
    src = torch.full((16384,), 77, dtype=torch.uint8, device="cuda")
    dst = torch.full((16384,), SENTINEL, dtype=torch.uint8, device="cuda")
    m01 = torch.full((4096,), float("nan"), dtype=torch.float32, device="cuda")

    def record(i=0, **kw):
        return SE.SelfensRecord(**dict(dict(src_off=4096 * i, dst_off=4096 * i, h=7 - i, w=5 + i, op=5 + i, pad=0), **kw))

    def transform(records=None, n=None, **kw):
        records = [record(0), record(1)] if records is None else records
        a = dict(dict(src=src.data_ptr(), dst=dst.data_ptr()), **kw)
        rc = lib.srgd_selfens_transform(a["src"], a["dst"], (SE.SelfensRecord * len(records))(*records), len(records) if n is None else n, _stream())
        return rc, lib.srgd_selfens_last_error().decode()

    def image(i=0, **kw):
        f = dict(dict(dst_off=4096 * i, mean01_off=1000 * i, H=7 - i, W=5 + i, n_src=2, src_off=[8192 * i, 8192 * i + 4096], op=[0, 5 + i]), **kw)
        im = SE.SelfensImage(f["dst_off"], f["mean01_off"], f["H"], f["W"], f["n_src"], 0)
        for j, (off, op) in enumerate(zip(f["src_off"], f["op"])):
            im.src_off[j], im.op[j] = off, op
        return im

    def merge(images=None, n=None, **kw):
        images = [image(0), image(1)] if images is None else images
        a = dict(dict(src=src.data_ptr(), dst=dst.data_ptr(), m01=m01.data_ptr()), **kw)
        rc = lib.srgd_selfens_merge(a["src"], a["dst"], a["m01"], (SE.SelfensImage * len(images))(*images), len(images) if n is None else n, _stream())
        return rc, lib.srgd_selfens_last_error().decode()
    every = [(transform, {"null": [dict(src=None), dict(dst=None)], "n must be": [dict(n=0)],
                          "bad size": [dict(records=[record(0), record(1, h=0)]), dict(records=[record(0, h=26755, w=26755), record(1)])],
                          "op outside": [dict(records=[record(0), record(1, op=8)]), dict(records=[record(0, op=-1), record(1)])],
                          "multiple of 16": [dict(records=[record(0), record(1, dst_off=4100)]), dict(records=[record(0, src_off=8), record(1)])],
                          "outside [0, 2^36)": [dict(records=[record(0), record(1, dst_off=-16)]), dict(records=[record(0, src_off=1 << 36), record(1)])],
                          "16-byte aligned": [dict(src=src.data_ptr() + 4), dict(dst=dst.data_ptr() + 8)],
                          "overlap": [dict(dst=src.data_ptr()), dict(dst=src.data_ptr() + 4096)]}),
             (merge, {"null": [dict(src=None), dict(dst=None)], "n_images": [dict(n=0)],
                      "n_src": [dict(images=[image(0), image(1, n_src=0)]), dict(images=[image(0, n_src=9), image(1)])],
                      "bad size": [dict(images=[image(0), image(1, W=0)])],
                      "op outside": [dict(images=[image(0), image(1, op=[0, 8])])],
                      "multiple of 16": [dict(images=[image(0), image(1, dst_off=4100)]), dict(images=[image(0, src_off=[0, 4100]), image(1)])],
                      "outside [0, 2^36)": [dict(images=[image(0, dst_off=1 << 36), image(1)])],
                      "negative mean01": [dict(images=[image(0), image(1, mean01_off=-1)])],
                      "16-byte aligned": [dict(src=src.data_ptr() + 4), dict(dst=dst.data_ptr() + 8)],
                      "4-byte aligned": [dict(m01=m01.data_ptr() + 2)],
                      "overlap": [dict(dst=src.data_ptr()), dict(dst=src.data_ptr() + 12288)]})]
    for call, cases in every:
        for phrase, calls in cases.items():
            for kw in calls:
                rc, msg = call(**kw)
                assert rc == -1 and phrase in msg, (call.__name__, phrase, kw, msg)
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all()) and bool((src == 77).all()) and bool(torch.isnan(m01).all())
    rc, msg = transform()                                                     # the same calls with nothing wrong in them run
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert bool((dst[:105] == 77).all()) and bool((dst[105:4096] == SENTINEL).all()) and bool((dst[4096:4096 + 108] == 77).all())
    assert bool((dst[4096 + 108:] == SENTINEL).all())
    dst.fill_(SENTINEL)
    rc, msg = merge()
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert bool((dst[:105] == 77).all()) and bool((dst[105:4096] == SENTINEL).all()) and bool((dst[4096:4096 + 108] == 77).all())
    unit = float(np.float32(77) / np.float32(255))
    assert bool((m01[:105] == unit).all()) and bool(torch.isnan(m01[105:1000]).all()) and bool((m01[1000:1108] == unit).all())
    with pytest.raises(ValueError, match="do not fit"):
        SE.transform_flat(src, [0, 16368], dst, [0, 4096], [(7, 5), (6, 6)], [0, 1])
    with pytest.raises(ValueError, match="do not fit"):
        SE.merge_flat(src, [[0, 16368]], [[0, 1]], dst, [0], [(7, 5)])


# ------------------------------------------------------------------------------------------- (c) the command line
def _lr(h, w, seed):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng([seed, h, w])
    base = np.stack([128 + 90 * np.sin(x / 5.0 + seed) * np.cos(y / 6.0), 100 + 4.0 * x - 2.5 * y, 140 + 60 * np.cos((x + y) / 4.0)], axis=2)
    return np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)


def test_cli_self_ensemble(tmp_path):
    """Three model runs and one refusal.  Run 1 (--self_ensemble 8) must equal the restatement's merge of run 2, a plain run over the
    16 numpy-transformed inputs as files of their own: a lock-step image is bit-identical to its solo run, whatever group it is in."""
    from srgd_amd.synth import synth_state_dict
    from tests.test_engine_gpu import _schema
    dim = 16
    conf_src = open(os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")).read()
    conf = tmp_path / "dim16.yaml"
    conf.write_text(conf_src.replace("unet_dim: 128", f"unet_dim: {dim}"))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"ema_model": synth_state_dict(_schema(dim), seed=3), "epoch": 300}, ckpt)
    indir, turned, gt = tmp_path / "in", tmp_path / "in_turned", tmp_path / "gt"
    for d in (indir, turned, gt):
        d.mkdir()
    lows = {"a": _lr(22, 24, 1), "b": _lr(24, 24, 2)}
    for name, x in lows.items():
        Image.fromarray(x, "RGB").save(indir / f"{name}.png")
        for op in range(8):
            Image.fromarray(SC.apply(x, op), "RGB").save(turned / f"{name}_op{op}.png")
        Image.fromarray(_lr(4 * x.shape[0], 4 * x.shape[1], 5), "RGB").save(gt / f"{name}.png")

    def run(outdir, *extra, source=indir):
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "-c", str(conf), "-m", str(ckpt), "--input_dir", str(source),
               "--output_dir", str(tmp_path / outdir), "--num_sample_steps", "2", "--test_label", "1", "--batch_size", "4", "--device_noise",
               "--seed", "71", "--lockstep_tiles", "16", *extra]
        return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)

    def png(outdir, name):
        with Image.open(tmp_path / outdir / name) as im:
            assert im.mode == "RGB"
            return np.asarray(im).copy()
    same = ("--color_fix", "wavelet", "--back_project", "1", "--consistency")
    first = run("plus", "--self_ensemble", "8", *same)                        # 1
    assert first.returncode == 0, first.stderr[-3000:]
    second = run("solo", *same, source=turned)                                # 2: only after the first returned 0
    assert second.returncode == 0, second.stderr[-3000:]
    assert sorted(os.listdir(tmp_path / "plus")) == ["a_out.png", "b_out.png", "consistency.json"]
    doc = json.load(open(tmp_path / "plus" / "consistency.json"))
    for name, x in lows.items():
        got = png("plus", f"{name}_out.png")
        outs = [png("solo", f"{name}_op{op}_out.png") for op in range(8)]
        assert [o.shape for o in outs] == [(4 * s[0], 4 * s[1], 3) for s in (SE.out_size(*x.shape[:2], op) for op in range(8))]
        assert got.shape == (4 * x.shape[0], 4 * x.shape[1], 3) and got.min() < got.max()
        assert np.array_equal(got, SC.merge(outs, list(range(8)))), name
        assert not np.array_equal(got, outs[0]), name                         # not the plain output of the untransformed input
        want = CS.consistency_on_device([torch.from_numpy(got).cuda()], [torch.from_numpy(x).cuda()])[0]
        assert doc["files"][f"{name}_out.png"] == want, name
    third = run("four", "--self_ensemble", "4", "--samples", "2", "--reference_dir", str(gt), "--crop_border", "2")      # 3
    assert third.returncode == 0, third.stderr[-3000:]
    written = ["a_out.png", "a_out_s1.png", "b_out.png", "b_out_s1.png"]
    assert sorted(os.listdir(tmp_path / "four")) == written + ["metrics.json"]
    doc = json.load(open(tmp_path / "four" / "metrics.json"))
    assert doc["crop_border"] == 2 and list(doc["files"]) == written and list(doc["images"]) == ["a.png", "b.png"]
    for name in written:
        saved = png("four", name)
        ref = torch.from_numpy(np.asarray(Image.open(gt / f"{name[0]}.png").convert("RGB")).copy()).cuda()
        want = MX.metrics_on_device(torch.from_numpy(SC.mean01(saved))[None].cuda(), ref, 2)[0]
        assert doc["files"][name] == want, name
    assert not np.array_equal(png("four", "a_out.png"), png("four", "a_out_s1.png"))
    refused = run("refused", "--self_ensemble", "3")                          # 4
    assert refused.returncode != 0 and "--self_ensemble" in refused.stderr and "engine ready" not in refused.stdout
    assert not os.path.exists(tmp_path / "refused")
