"""``--back_project``, host side (no GPU): the yardstick itself (tests/backproject_cases.py: Pillow's two resizes and a clip) on hand
cases and on every planned GPU input (the clip acts both ways and LR-MSE falls in every one of five iterations: the GPU comparisons
are not vacuous), the two quantisations, the sixteen coefficient vectors of the library against Pillow's formula and the
sixteen-vector fact the update kernel rests on, the C-ABI declarations, exports and refusals of the new library, the module's own
checks, the resource table of the new kernels, the flag, the keywords and the batch loop with fake samplers."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import pil_resample as PR
from srgd_amd import _lib
from srgd_amd import backproject as BP
from srgd_amd import consistency as CS
from srgd_amd import ensemble as EN
from srgd_amd import inference as INF
from srgd_amd import metrics as MX
from srgd_amd import model as MODEL
from tests import backproject_cases as B
from tests import consistency_cases as K
from tests.lib_exports import exports as _exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")
ENTRIES = {"srgd_image_backproject", "srgd_image_backproject_images", "srgd_image_backproject_coeffs", "srgd_image_backproject_last_error"}


def _argv(*extra):
    return ["-c", CONF, "-m", "ckpt.pth", "--input_dir", "in", "--output_dir", "out", *extra]


# ------------------------------------------------------------------------------------------- the yardstick
def test_hand_cases_of_the_yardstick():
    # a constant a reduces to a and enlarges to a (every coefficient row sums to 1 << 22): O + C - U = a + b - a = b, and b stays
    for a, b in ((0, 255), (255, 0), (17, 200), (200, 17), (128, 128), (0, 0), (255, 255)):
        out, cond = K.constant(20, 28, a), K.constant(20, 28, b)
        seq = B.steps(out, cond, 3)
        assert all((o == b).all() for o in seq[1:]), (a, b)
        assert np.array_equal(B.raw_step(out, cond), np.full((20, 28, 3), b, dtype=np.int64))
    lr = K.random_pair(6, 7, 3)[1]
    cond = K.pillow_up(lr)
    one = B.step(cond, cond)
    assert one.dtype == np.uint8 and one.shape == cond.shape
    assert np.array_equal(one.astype(np.int64), np.clip(2 * cond.astype(np.int64) - K.pillow_up(K.pillow_down(cond)), 0, 255))


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("h,w", B.SIZES)
def test_on_every_gpu_input_the_clip_acts_both_ways_and_lr_mse_falls_in_every_iteration(h, w, kind):
    out, cond, lr, seq = B.case(kind, h, w)
    assert len(seq) == 6 and seq[0] is out and cond.shape == out.shape == (4 * h, 4 * w, 3)
    mse = [K.yardstick(o, lr)[2]["lr_mse"] for o in seq]
    for k in range(5):
        raw = B.raw_step(seq[k], cond)
        assert (raw < 0).any() and (raw > 255).any(), (k, int(raw.min()), int(raw.max()))
        assert np.array_equal(seq[k + 1], np.clip(raw, 0, 255))
        assert mse[k + 1] < mse[k], (k, mse)


def test_a_colour_shift_is_pulled_back():
    # a plausible output: a smooth image's condition with a colour shift - the first iteration brings it closer to its input, no later one away
    y, x = np.mgrid[0:31, 0:65]
    lr = np.stack([60 + 2 * x, 200 - 3 * y, 90 + x + y], axis=2).astype(np.uint8)
    cond = K.pillow_up(lr)
    out = np.clip(cond.astype(np.int64) + np.array([12, -9, 5]), 0, 255).astype(np.uint8)
    psnr = [K.yardstick(o, lr)[2]["lr_psnr"] for o in B.steps(out, cond, 3)]
    assert psnr[0] < psnr[1] and all(a <= b for a, b in zip(psnr, psnr[1:])), psnr


# ------------------------------------------------------------------------------------------- the two quantisations
def test_the_two_quantisations():
    u8 = np.arange(256, dtype=np.uint8)
    unit = u8.astype(np.float32) / np.float32(255)
    assert np.array_equal(B.quant_cond(unit), u8) and np.array_equal(B.quant_out(unit), u8)
    img = np.random.default_rng(6).integers(0, 256, (8, 12, 3), dtype=np.uint8)
    assert B.unit(img).shape == (3, 8, 12) and np.array_equal(B.quant_out(B.unit(img)).transpose(1, 2, 0), img)
    # q is the saved file on [0,1]: mul(255) and truncation (oracle.pil_resample.to_u8_hwc)
    v = np.random.default_rng(5).random((3, 9, 11), dtype=np.float32)
    v[0, 0, :4] = [0.0, 1.0, np.float32(1 / 255), np.nextafter(np.float32(1), np.float32(0))]
    assert np.array_equal(B.quant_out(v).transpose(1, 2, 0), PR.to_u8_hwc(v))
    # ... and saturates outside it, where the saved file wraps; r rounds half up
    odd = np.array([-0.3, 1.7, -0.0, np.nan, np.inf, -np.inf, 1e30, -1e30, 0.5, 0.9999, 254.5 / 255], dtype=np.float32)
    assert B.quant_out(odd).tolist() == [0, 255, 0, 0, 255, 0, 255, 0, 127, 254, 254]
    assert B.quant_cond(odd).tolist() == [0, 255, 0, 0, 255, 0, 255, 0, 128, 255, 255]
    assert PR.to_u8_hwc(np.full((3, 1, 1), 1.7, dtype=np.float32)).ravel().tolist() != [255, 255, 255]


# ------------------------------------------------------------------------------------------- coefficients
def _vector(j, n):
    """The row of the sixteen-vector table that output index j of 4n uses."""
    return j if j < 6 else (10 + j - (4 * n - 6) if j >= 4 * n - 6 else 6 + (j - 6) % 4)


def test_the_librarys_sixteen_vectors_are_pillows_rows():
    got = BP.coeffs()
    bounds, kk = PR.precompute_coeffs(64, 256)
    assert kk.shape == (256, 5) and not kk[:, 4].any()
    rows = list(range(10)) + list(range(250, 256))
    assert len(got) == 16 and all(len(v) == 4 for v in got)
    for vec, row in zip(got, rows):
        assert vec == kk[row, :4].tolist(), row
    assert [int(bounds[r, 1]) for r in rows] == [2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 3, 3, 3, 3, 2, 2]
    assert all(abs(sum(v) - (1 << 22)) <= 2 for v in got)         # every vector sums to one, up to the rounding of its taps
    assert max(abs(v) for vec in got for v in vec) < 1 << 23     # a tap is a 24-bit multiply in the kernel
    assert BP.lib().srgd_image_backproject_coeffs(None) == -1
    assert BP.lib().srgd_image_backproject_last_error().decode().startswith("srgd_image_backproject_coeffs: ")


@pytest.mark.parametrize("n", list(range(5, 70)) + [100, 257])
def test_the_sixteen_vector_fact(n):
    table = np.array(BP.coeffs(), dtype=np.int64)
    bounds, kk = PR.precompute_coeffs(n, 4 * n)
    kk = kk.astype(np.int64)
    assert kk.shape == (4 * n, 5) and not kk[:, 4].any()
    assert [bounds[j].tolist() for j in range(6)] == [[0, 2], [0, 2], [0, 3], [0, 3], [0, 3], [0, 3]]
    assert [bounds[4 * n - 6 + j].tolist() for j in range(6)] == [[n - 3, 3]] * 4 + [[n - 2, 2]] * 2
    for j in range(4 * n):
        assert np.array_equal(kk[j, :4], table[_vector(j, n)]), j
        if 6 <= j < 4 * n - 6:
            assert bounds[j].tolist() == [(j - 6) // 4, 4], j
    # the end vectors are mirror images of the first six, the phases of each other
    for j in range(6):
        taps = int(bounds[j, 1])
        assert np.array_equal(table[15 - j, :taps], table[j, :taps][::-1])
    assert np.array_equal(table[6], table[9][::-1]) and np.array_equal(table[7], table[8][::-1])


# ------------------------------------------------------------------------------------------- C ABI, refusals, resources
def test_entries_are_declared_prototyped_and_exported_by_a_library_of_their_own():
    header = open(os.path.join(ROOT, "include", "srgd_backproject.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(srgd_[a-z0-9_]+)\s*\(", flat))
    assert declared == ENTRIES == set(BP.PROTOTYPES)
    for name, (_, argtypes) in BP.PROTOTYPES.items():
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", flat).group(1).strip()
        assert (0 if params == "void" else len(params.split(","))) == len(argtypes), name
    assert os.path.exists(BP.LIB_PATH), "build the library first (python -m srgd_amd.build)"
    assert _exports(BP.LIB_PATH) == ENTRIES
    assert BP.lib().srgd_image_backproject_last_error() is not None            # binds every prototype
    # the four other libraries: their exports are what their modules prototype, and none holds a back-projection name
    for mod in (_lib, MX, EN, CS):
        assert _exports(mod.LIB_PATH) == set(mod.PROTOTYPES), mod.__name__
        assert not any("backproject" in n for n in _exports(mod.LIB_PATH)), mod.__name__
        assert not set(BP.PROTOTYPES) & set(mod.PROTOTYPES)
    assert not any("metrics" in n or "ensemble" in n or "consistency" in n for n in ENTRIES)
    for phrase in ("out01 and cond01 are fp32 planar [3][H][W], H = 4h, W = 4w, h, w >= 5, 48*h*w < 2^31 - 256",
                   "t = fmul_rn(v, 255);  q = 0 if t is NaN or t <= 0, q = 255 if t >= 255, otherwise q = (int)t, truncated",
                   "outside [0,1] it saturates where the saved file wraps",
                   "r = 0 for NaN, otherwise r = clamp((int)floorf(fmul_rn(v, 255) + 0.5f), 0, 255)",
                   "D = Pillow Image.resize((w, h), BICUBIC) of O_{k-1}", "U = Pillow Image.resize((W, H), BICUBIC) of D",
                   "src/libImaging/Resample.c", "support 2, a = -0.5", "window clipped to the image and renormalised",
                   "O_k = clip(O_{k-1} + C - U, 0, 255)", "dst01 = fdiv_rn((float)O_N, 255)",
                   "Elements where out01 was non-finite receive out01's value unchanged",
                   "O (48*h*w bytes) + C (48*h*w bytes) + D (3*h*w bytes), each rounded up to a multiple of 256 bytes",
                   "dst01 == out01 is allowed and means in place"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", header), phrase


def test_refusals_need_no_gpu():
    # every refusal is decided on the host before anything is launched, so it can be checked here: -1 and a message
    lib = BP.lib()
    off, hw = (C.c_int64 * 1)(0), (C.c_int32 * 2)(5, 5)
    span = 4 * 48 * 5 * 5                                  # bytes of a 5x5 image's planes
    # never dereferenced: a refused call launches nothing.  out01, cond01, dst01 three ranges apart, the scratch 256-byte aligned
    out, cond, dst, scr = (C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20))
    ok = dict(out=out, cond=cond, offs=off, hw=hw, n=1, it=3, dst=dst, scratch=scr)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.srgd_image_backproject_images(a["out"], a["cond"], a["offs"], a["hw"], a["n"], a["it"], a["dst"], a["scratch"], None)
        return rc, lib.srgd_image_backproject_last_error().decode()
    size = lambda h, w: (C.c_int32 * 2)(h, w)              # noqa: E731
    one = lambda v: (C.c_int64 * 1)(v)                     # noqa: E731
    at = lambda v: C.c_void_p(v)                           # noqa: E731
    cases = {"null": [dict(out=None), dict(cond=None), dict(offs=None), dict(hw=None), dict(dst=None), dict(scratch=None)],
             "n_images": [dict(n=0), dict(n=-1)],
             "iterations": [dict(it=0), dict(it=-1), dict(it=65)],
             "bad size": [dict(hw=size(4, 5)), dict(hw=size(5, 4)), dict(hw=size(0, 9)), dict(hw=size(9, -1))],
             "2^31 - 256": [dict(hw=size(6689, 6689)), dict(hw=size(5, 8947848))],
             "offset outside": [dict(offs=one(-1)), dict(offs=one(-4096))],
             "4-byte aligned": [dict(out=at((1 << 20) + 2)), dict(cond=at((2 << 20) + 1)), dict(dst=at((3 << 20) + 3))],
             "256-byte aligned": [dict(scratch=at((4 << 20) + 128)), dict(scratch=at((4 << 20) + 16))],
             "partial overlap of dst01 and out01": [dict(dst=at((1 << 20) + 4)), dict(dst=at((1 << 20) - 4)), dict(dst=at((1 << 20) + span - 4)),
                                                    dict(dst=at((1 << 20) - span + 4))],
             "overlap of dst01 and cond01": [dict(dst=cond), dict(dst=at((2 << 20) + 4)), dict(dst=at((2 << 20) - span + 4)),
                                             dict(cond=out, dst=out)]}
    for word, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == -1 and word in msg and msg.startswith("srgd_image_backproject_images: "), (kw, msg)
    rc = lib.srgd_image_backproject(out, cond, 4, 9, 3, dst, scr, None)
    assert rc == -1 and lib.srgd_image_backproject_last_error().decode().startswith("srgd_image_backproject: bad size")
    rc = lib.srgd_image_backproject(out, cond, 5, 5, 0, dst, scr, None)
    assert rc == -1 and "iterations" in lib.srgd_image_backproject_last_error().decode()
    # a bad image anywhere in the group refuses the whole call
    rc = lib.srgd_image_backproject_images(out, cond, (C.c_int64 * 2)(0, 4800), (C.c_int32 * 4)(5, 5, 5, 4), 2, 3, dst, scr, None)
    assert rc == -1 and "bad size" in lib.srgd_image_backproject_last_error().decode()
    assert 48 * 5 * 8947848 == 2 ** 31 - 128 and 48 * 5 * 8947847 < 2 ** 31 - 256 <= 48 * 5 * 8947848     # the first refused width at h = 5
    assert 48 * 6689 * 6689 >= 2 ** 31 - 256 > 48 * 6688 * 6688


def test_host_side_checks_of_the_module():
    assert (BP.MIN_SIDE, BP.SCALE, BP.MAX_ITERATIONS, BP.ALIGN) == (5, 4, 64, 256)
    # the header's scratch formula: O and C of 48hw bytes and D of 3hw bytes, each rounded up to 256
    assert BP.scratch_bytes([(5, 5)]) == 2 * 1280 + 256 and BP.scratch_bytes([(16, 16)]) == 2 * 12288 + 768
    assert BP.scratch_bytes([(31, 65), (5, 37)]) == (2 * 96768 + 6144) + (2 * 8960 + 768)
    with pytest.raises(ValueError, match="size"):
        BP.scratch_bytes([(4, 40)])
    assert BP.check_iterations(None) is None and BP.check_iterations(0) is None
    assert BP.check_iterations(1) == 1 and BP.check_iterations(64) == 64
    for bad in (-1, 65, 2.0, "3", True):
        with pytest.raises(ValueError, match="iterations"):
            BP.check_iterations(bad)
    assert BP.check_hr_sizes([(20, 28), (1024, 1024)]) == [(5, 7), (256, 256)]
    for bad in ((16, 40), (40, 16), (22, 40), (40, 41), (300, 302), (4 * 6689, 4 * 6689)):
        with pytest.raises(ValueError, match="bad image size"):
            BP.check_hr_sizes([(20, 20), bad])
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32)            # noqa: E731
    for out, cond in ((f32(3, 20, 20), f32(3, 20, 24)), (f32(20, 20), f32(20, 20)), (f32(2, 4, 20, 20), f32(2, 4, 20, 20)),
                      (f32(1, 3, 20, 20), [f32(1, 3, 20, 20)]), ([], []), ([f32(1, 3, 20, 20)], [f32(1, 3, 20, 20)] * 2),
                      ([f32(3, 20, 20)], [f32(3, 20, 20)]), ([f32(1, 3, 20, 20), "x"], [f32(1, 3, 20, 20)] * 2), (None, None),
                      (f32(3, 16, 40), f32(3, 16, 40)), (f32(1, 3, 40, 22), f32(1, 3, 40, 22)), ([f32(1, 3, 24, 18)], [f32(1, 3, 24, 18)])):
        with pytest.raises(ValueError, match="back_project"):
            BP.back_project_on_device(out, cond, 3)
    for bad in (0, None, 65, -2):
        with pytest.raises(ValueError, match="iterations"):
            BP.back_project_on_device(f32(3, 20, 20), f32(3, 20, 20), bad)
        with pytest.raises(ValueError, match="iterations"):
            BP.back_project_flat(f32(1200), f32(1200), [0], [(20, 20)], bad)
    for out, cond in ((f32(3, 20, 20), f32(3, 20, 20)), (f32(2, 3, 20, 28), f32(2, 3, 20, 28)), ([f32(1, 3, 20, 20)], [f32(1, 3, 20, 20)])):
        with pytest.raises(_lib.SrgdHipError, match="no CPU fallback"):      # a missing GPU is an error, never another path
            BP.back_project_on_device(out, cond, 3)
    with pytest.raises(_lib.SrgdHipError, match="no CPU fallback"):
        BP.back_project_flat(f32(1200), f32(1200), [0], [(20, 20)], 1)
    assert list(inspect.signature(BP.back_project_flat).parameters) == ["out", "cond", "offsets", "sizes", "iterations", "dst"]
    assert inspect.signature(BP.back_project_flat).parameters["dst"].default is None
    assert list(inspect.signature(BP.back_project_on_device).parameters) == ["out", "cond", "iterations"]
    assert list(inspect.signature(BP.scratch_bytes).parameters) == ["sizes"] and list(inspect.signature(BP.check_iterations).parameters) == ["n"]


def test_backproject_kernels_do_not_spill_and_fit_four_workgroups_per_cu():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_table
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "backproject.hip")) if "backproject_" in r["name"]]
    assert sorted(r["name"] for r in rows) == ["backproject_begin_kernel", "backproject_end_kernel", "backproject_reduce_kernel",
                                               "backproject_update_kernel"]
    for r in rows:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["lds"] <= 160 * 1024 // 4 and r["vgpr"] <= 128, r       # four 256-thread workgroups per CU: LDS and registers
    lds = {r["name"]: r["lds"] for r in rows}
    assert lds["backproject_reduce_kernel"] == 72 * 448 + 72 * 96 + 320
    assert lds["backproject_update_kernel"] == 19 * 112 + 19 * 384 + 256
    assert lds["backproject_begin_kernel"] == 0 and lds["backproject_end_kernel"] == 0


# ------------------------------------------------------------------------------------------- flag and keywords
def test_the_flag_parses_and_the_entry_is_reexported():
    assert INF.parse_args(_argv()).back_project == 0
    assert INF.parse_args(_argv("--back_project", "3")).back_project == 3
    assert INF.parse_args(_argv("--back_project", "0")).back_project == 0 and INF.parse_args(_argv("--back_project", "64")).back_project == 64
    args = INF.parse_args(_argv("--back_project", "5", "--consistency", "--samples", "3", "--ensemble", "--reference_dir", "gt",
                                "--color_fix", "wavelet"))
    assert args.back_project == 5 and args.consistency is True and args.color_fix == "wavelet"
    for bad in ("-1", "65", "1000"):
        with pytest.raises(SystemExit, match="--back_project"):
            INF.parse_args(_argv("--back_project", bad))
    with pytest.raises(SystemExit):
        INF.parse_args(_argv("--back_project", "two"))
    assert INF.back_project_on_device is BP.back_project_on_device


def test_every_keyword_defaults_to_zero():
    for fn in (INF.sr_target_image, INF.sr_target_images, INF.sr_target_images_mixed, INF.sr_target_images_seeded,
               INF.batch_sr_target_images, MODEL.ConditionalContinuousTimeGaussianDiffusionSR.tiled_sample,
               MODEL.ConditionalElucidatedDiffusionSR.tiled_sample):
        assert inspect.signature(fn).parameters["back_project"].default == 0, fn.__qualname__
    assert INF._back_project_kw(0) == {} and INF._back_project_kw(None) == {} and INF._back_project_kw(3) == {"back_project": 3}


class _Unused:
    """A sampler whose every attribute access fails the test: ``tiled_sample`` must refuse before it touches the model."""
    canvas_group = None

    def __getattr__(self, name):
        raise AssertionError(f"the sampler was touched ({name}) before the sizes were checked")


@pytest.mark.parametrize("cls", ["ConditionalContinuousTimeGaussianDiffusionSR", "ConditionalElucidatedDiffusionSR"])
def test_tiled_sample_checks_the_keyword_and_the_sizes_on_entry(cls):
    fn = inspect.unwrap(getattr(MODEL, cls).tiled_sample)
    for bad in (-1, 65, 1.5):
        with pytest.raises(ValueError, match="iterations"):
            fn(_Unused(), condition_x=torch.zeros(1, 3, 256, 256), back_project=bad)
    for shape in ((1, 3, 300, 302), (2, 3, 16, 64), (1, 3, 258, 256)):
        with pytest.raises(ValueError, match="bad image size"):
            fn(_Unused(), condition_x=torch.zeros(*shape), back_project=3)
    with pytest.raises(ValueError, match="bad image size"):
        fn(_Unused(), condition_x=[torch.zeros(1, 3, 256, 256), torch.zeros(1, 3, 64, 30)], back_project=1)


# ------------------------------------------------------------------------------------------- the batch loop
def _fake_samplers(monkeypatch, calls):
    def fake(kind):
        def run(images, *a, **kw):
            ims = images if isinstance(images, list) else [images]
            calls.append((kind, len(ims), dict(kw)))
            outs = [Image.fromarray(np.zeros((im.size[1] * 4, im.size[0] * 4, 3), dtype=np.uint8), "RGB") for im in ims]
            return outs if isinstance(images, list) else outs[0]
        return run
    monkeypatch.setattr(INF, "sr_target_image", fake("solo"))
    monkeypatch.setattr(INF, "sr_target_images", fake("same"))
    monkeypatch.setattr(INF, "sr_target_images_mixed", fake("mixed"))
    monkeypatch.setattr(INF, "sr_target_images_seeded", fake("seeded"))


def test_the_batch_loop_hands_the_keyword_on_only_when_it_is_set(tmp_path, monkeypatch):
    calls = []
    _fake_samplers(monkeypatch, calls)
    indir = tmp_path / "in"
    indir.mkdir()
    rng = np.random.default_rng(0)
    for name, (w, h) in {"a": (64, 64), "b": (64, 64), "c": (48, 64)}.items():
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(indir / f"{name}.png")
    run = lambda tag, **kw: INF.batch_sr_target_images(str(indir), str(tmp_path / tag), None, seed=71, **kw)  # noqa: E731
    for tag, kw in (("solo", {}), ("same", dict(lockstep=2)), ("mixed", dict(lockstep_tiles=8)), ("seeded", dict(samples=2))):
        calls.clear()
        run(tag + "_off", **kw)
        run(tag + "_zero", back_project=0, **kw)
        assert calls and all("back_project" not in c[2] for c in calls), tag
        kinds_off = [c[:2] for c in calls[:len(calls) // 2]]
        calls.clear()
        run(tag + "_on", back_project=3, **kw)
        assert [c[:2] for c in calls] == kinds_off and all(c[2]["back_project"] == 3 for c in calls), tag
        assert sorted(os.listdir(tmp_path / (tag + "_on"))) == sorted(os.listdir(tmp_path / (tag + "_off")))
