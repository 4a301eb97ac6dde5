"""Mixed-size lock-step, host side: the CLI's grouping under a tile budget, the per-image geometry records, the noise classes,
the new C-ABI entry and the resource table of the sampler kernels that now address through the image records (no GPU)."""
import json
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_groups_respect_the_tile_budget_and_file_order():
    from srgd_amd.lockstep import even_step_tiles, plan_lockstep_groups
    assert even_step_tiles(480, 320) == 9 and even_step_tiles(320, 480) == 9 and even_step_tiles(256, 256) == 1
    bsd = [(480, 320), (320, 480)] * 10                         # BSD100 x4 shapes: 9 even tiles each
    groups = plan_lockstep_groups(bsd, 125)
    assert [len(g) for g in groups] == [13, 7]                  # 13 * 9 = 117 <= 125 < 126
    assert [i for g in groups for i in g] == list(range(20))    # file order kept, nothing dropped
    assert plan_lockstep_groups(bsd[:4], 18) == [[0, 1], [2, 3]]   # at the budget exactly: the group stays open
    # an image above the budget runs alone; its neighbours are not merged across it
    sizes = [(256, 256), (256, 256), (2048, 2048), (256, 256)]
    assert even_step_tiles(2048, 2048) == 81
    assert plan_lockstep_groups(sizes, 64) == [[0, 1], [2], [3]]
    assert plan_lockstep_groups([(2048, 2048)], 1) == [[0]]
    assert plan_lockstep_groups([], 64) == []


def test_image_records_are_the_solo_geometry():
    from srgd_amd.lockstep import plan_mixed_group
    from srgd_amd.model import get_area, get_coord_and_pad, get_coords
    from tests.golden import cases as C
    with open(os.path.join(G, "geometry.json")) as f:
        geo = json.load(f)
    def solo_ok(h, w):                                           # sizes whose reflect pad a solo run accepts
        _, pad = get_coord_and_pad(h, w)
        return max(pad[0], pad[1]) < w and max(pad[2], pad[3]) < h
    sizes = [s for s in C.GEOMETRY_SIZES if s[0] * s[1] <= 1500 * 1500 and solo_ok(*s)] + [(480, 320), (320, 480), (384, 384)]
    plans, _ = plan_mixed_group(sizes)
    covered = 0
    for (h, w), p in zip(sizes, plans):
        box, pad = get_coord_and_pad(h, w)
        hp, wp = h + pad[2] + pad[3], w + pad[0] + pad[1]
        even = get_coords(hp, wp, 256, 256, diff=0)
        odd = even if (hp <= 256 and wp <= 256) else get_coords(hp - 256, wp - 256, 256, 256, diff=128)
        inner, _ = get_area(odd, hp, wp)
        assert (p.H, p.W, p.Hp, p.Wp) == (h, w, hp, wp)
        assert p.box == tuple(box) and p.inner == tuple(inner)
        assert p.coords0 == even and p.coords1 == odd
        want = geo.get(f"{h}x{w}")
        if want is not None:                                     # the reference's own numbers where the table holds the size
            covered += 1
            assert list(p.box) == want["box"] and [p.Hp, p.Wp] == want["canvas"] and list(p.inner) == want["inner"]
            assert len(p.coords0) == want["n_even"] and len(p.coords1) == want["n_odd"]
            if not want["truncated"]:
                assert [list(c) for c in p.coords0] == want["even"] and [list(c) for c in p.coords1] == want["odd"]
    assert covered >= 5


def test_noise_classes_are_canvas_sizes():
    from srgd_amd.lockstep import plan_mixed_group
    plans, classes = plan_mixed_group([(480, 320), (256, 256), (320, 480), (1024, 1024), (384, 384), (480, 320)])
    assert classes == [(768, 768), (256, 256), (1280, 1280)]    # in order of first appearance
    assert [p.noise_class for p in plans] == [0, 1, 0, 2, 0, 0]  # 480x320, 320x480 and 384^2 all pad to 768^2
    assert plans[1].noise_class != plans[3].noise_class          # 256^2 and 1024^2 do not share
    with pytest.raises(RuntimeError, match="Padding size"):      # a reflect pad F.pad refuses, as for a solo run
        plan_mixed_group([(256, 256), (100, 300)])


def test_mixed_begin_is_exported_and_declared():
    from srgd_amd import _lib
    from srgd_amd.build import build
    build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srgd_hip.h")).read(), flags=re.S)
    assert re.search(r"\bsrgd_sampler_begin_images\s*\(", text)
    assert "srgd_sampler_begin_images" in _lib.PROTOTYPES
    assert hasattr(_lib.lib(), "srgd_sampler_begin_images")
    import ctypes as C
    assert C.sizeof(_lib.SamplerImage) == 13 * 4


def test_cli_lockstep_flags():
    from srgd_amd.inference import parse_args
    base = ["-c", "x", "-m", "w", "--input_dir", "i", "--output_dir", "o"]
    a = parse_args(base)
    assert a.lockstep == 1 and a.lockstep_tiles is None
    assert parse_args(base + ["--lockstep_tiles", "125"]).lockstep_tiles == 125
    with pytest.raises(SystemExit):
        parse_args(base + ["--lockstep_tiles", "64", "--lockstep", "4"])


def test_cli_groups_skip_existing_and_unreadable_files(tmp_path, monkeypatch, capsys):
    # the folder walk of batch_sr_target_images with the sampling replaced: which files form which group
    from PIL import Image
    import srgd_amd.inference as I
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    dst.mkdir()
    sizes = {"a": (120, 80), "b": (80, 120), "c": (64, 64), "d": (120, 80), "e": (512, 512), "f": (80, 120)}
    for name, wh in sizes.items():
        Image.new("RGB", wh, (10, 20, 30)).save(src / f"{name}.png")
    (src / "bad.png").write_bytes(b"not an image")               # unreadable: not counted
    Image.new("RGB", (8, 8)).save(dst / "c_out.png")             # output exists: skipped, not counted
    calls = []

    def fake_many(images, sr_model, **kw):
        calls.append([im.size for im in images])
        return [Image.new("RGB", (w * 4, h * 4)) for (w, h) in (im.size for im in images)]

    def fake_one(image, sr_model, **kw):
        return fake_many([image], sr_model, **kw)[0]
    monkeypatch.setattr(I, "sr_target_images_mixed", fake_many)
    monkeypatch.setattr(I, "sr_target_image", fake_one)
    I.batch_sr_target_images(str(src), str(dst), sr_model=None, lockstep_tiles=20)
    # a, b (9 + 9) | bad, c not counted | d, e: e is 2048^2 = 81 tiles -> alone | f
    assert calls == [[(120, 80), (80, 120)], [(120, 80)], [(512, 512)], [(80, 120)]]
    out = capsys.readouterr().out
    assert "lock-step group: 2 images, 18 tiles per even step" in out
    assert "skip" in out and "Invalid image" in out
    assert sorted(os.listdir(dst)) == sorted(f"{n}_out.png" for n in sizes)


def test_sampler_kernels_do_not_spill():
    # the kernels that address through the image records (the two already in tests/test_kernel_resources_cpu.py + the canvas kernels)
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    sys.path.insert(0, ROOT)
    from tools.kernel_resources import kernel_table
    rows = kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "sampler.hip"))
    for key in ("final_step_kernel", "init_gather_kernel", "canvas_ring_renoise_kernel", "canvas_prepare_cond_kernel",
                "canvas_q_start_kernel", "canvas_finish_kernel"):
        hit = [r for r in rows if key in r["name"]]
        assert hit, key
        for r in hit:
            assert r["spill"] == 0 and r["scratch"] == 0, r
            assert 0 < r["vgpr"] <= 128, r
