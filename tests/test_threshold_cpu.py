"""The dynamic threshold, host side (no GPU): the library's quantile position against the restatement of tests/threshold_cases.py, the
restatement's order statistics against ``np.sort`` and its threshold against ``np.quantile`` in float64, the C-ABI declarations,
exports and refusals of the new library, the engine's one new switch, the module's own checks, the resource table of the new kernels
and of the step kernel, the flag, the keywords and what is refused."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from srgd_amd import _lib
from srgd_amd import guidance as GD
from srgd_amd import inference as INF
from srgd_amd import model as MODEL
from srgd_amd import solver as SV
from srgd_amd import threshold as TH
from tests import threshold_cases as TC
from tests.lib_exports import exports as _exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")
ENTRIES = {"srgd_threshold_step", "srgd_threshold_position", "srgd_threshold_scratch_bytes", "srgd_threshold_chunk_elems",
           "srgd_threshold_last_error"}


def _argv(*extra):
    return ["-c", CONF, "-m", "ckpt.pth", "--input_dir", "in", "--output_dir", "out", *extra]


# ------------------------------------------------------------------------------------------- positions and the restatement
def test_the_librarys_positions_are_the_restatements():
    for q in TC.QS:
        for n in list(range(1, 301)) + [2 ** 24 + 1, 2 ** 31 - 1]:
            lo, hi, frac = TH.position(n, q)
            want = TC.position_np(n, q)
            assert (lo, hi) == want[:2] and np.float32(frac).tobytes() == want[2].tobytes(), (n, q)
            assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and 0.0 <= frac <= 1.0
    assert TH.position(105, 0.5) == (52, 53, 0.0) and TH.position(7, 1.0) == (6, 6, 0.0) and TH.position(1, 0.5) == (0, 0, 0.0)
    assert TH.position(2 ** 31 - 1, 1.0)[:2] == (2 ** 31 - 2, 2 ** 31 - 2)
    for n, q in ((0, 0.5), (-3, 0.5), (10, 0.0), (10, -0.5), (10, 1.5), (10, float("nan")), (10, float("inf"))):
        with pytest.raises(_lib.SrgdHipError, match="srgd_threshold_position: "):
            TH.position(n, q)
    assert TH.lib().srgd_threshold_position(5, 0.5, None, None, None) == -1


@pytest.mark.parametrize("q", TC.QS)
@pytest.mark.parametrize("n", [1, 2, 105, 1000, 4097])
def test_the_restatement_selects_what_sorting_selects_and_interpolates_as_numpy_does(n, q):
    rng = np.random.default_rng([n, int(q * 1e6)])
    v = (rng.standard_normal(n) * 1.3).astype(np.float32)
    a_lo, a_hi, s_raw, s = TC.select_np(v, q)
    lo, hi, _ = TC.position_np(n, q)
    ordered = np.sort(TC.keys_of(v))
    assert a_lo.view(np.uint32) == ordered[lo] and a_hi.view(np.uint32) == ordered[hi]
    want = np.quantile(np.abs(v.astype(np.float64)), float(np.float32(q)))
    assert abs(float(s_raw) - want) <= float(np.spacing(np.float32(want))), (float(s_raw), want)
    assert s == max(np.float32(1), s_raw)


def test_the_keys_order_zeros_denormals_infinities_and_nans():
    v = np.array([np.nan, -np.inf, 3.0, -2.0, 1e-40, -1e-41, 0.0, -0.0], dtype=np.float32)
    k = TC.keys_of(v)
    assert k[6] == k[7] == 0 and k[5] < k[4] < k[3] < k[2] < k[1] < k[0]
    assert TC.select_np(np.array([0.5, -3.0, np.nan], dtype=np.float32), 1.0)[0].view(np.uint32) == k[0]       # NaNs sort last
    assert np.isnan(TC.select_np(np.array([0.5, -3.0, np.nan], dtype=np.float32), 1.0)[3])
    assert TC.select_np(np.array([0.5, -3.0, 2.0, 1.0, np.nan], dtype=np.float32), 0.5)[3] == np.float32(2.0)   # hi = 3: below the NaN
    assert np.isnan(TC.select_np(np.array([0.5, -3.0, np.nan], dtype=np.float32), 0.5)[3])                    # frac = 0, hi is the NaN: 0 * NaN


def test_the_restated_update_is_the_static_clamp_at_s_one_and_leaves_img_alone_where_nothing_changed():
    recs, img, xs, q = TC.KERNEL_CASES["quantile_below_1"](4096)
    img0, xs0 = img.copy(), xs.copy()
    s = TC.threshold_np(img, xs, recs, q, TC.WEIGHT)
    assert s.tolist() == [1.0]
    inside = np.zeros(xs.size, dtype=bool)
    TC.update_box(inside, recs[0])[...] = True
    assert np.array_equal(xs[inside], np.clip(xs0[inside], -1, 1)) and np.array_equal(xs[~inside], xs0[~inside])
    moved = inside & (np.abs(xs0) > 1)
    assert moved.sum() > 20 and np.array_equal(img[~moved].view(np.uint32), img0[~moved].view(np.uint32)) and (img[moved] != img0[moved]).all()


def test_every_kernel_case_builds_and_sits_between_canaries():
    chunk = TH.chunk_elems()
    sizes = {}
    for name, make in TC.KERNEL_CASES.items():
        recs, img, xs, q = make(chunk)
        assert 0 < q <= 1 and img.dtype == xs.dtype == np.float32 and img.shape == xs.shape
        covered = np.zeros(img.size, dtype=bool)
        for r in recs:
            assert r[0] > 0 and not covered[r[0]:r[0] + 3 * r[1] * r[2]].any()
            covered[r[0]:r[0] + 3 * r[1] * r[2]] = True
        assert (img[~covered] == TC.SENTINEL).all() and (~covered).sum() >= 7
        TH.records(recs)
        sizes[name] = 3 * recs[0][5] * recs[0][6]
    assert (sizes["chunk_minus_1"], sizes["chunks_exactly"], sizes["chunks_plus_1"]) == (chunk - 1, 3 * chunk, 2 * chunk + 1)
    assert chunk == 4096 and len(TC.KERNEL_CASES["many"](chunk)[0]) == 130


# ------------------------------------------------------------------------------------------- the library
def test_entries_are_declared_prototyped_and_exported_by_a_library_of_their_own():
    header = open(os.path.join(ROOT, "include", "srgd_threshold.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(srgd_[a-z0-9_]+)\s*\(", flat))
    assert declared == ENTRIES == set(TH.PROTOTYPES)
    for name, (_, argtypes) in TH.PROTOTYPES.items():
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", flat).group(1).strip()
        assert (0 if params == "void" else len(params.split(","))) == len(argtypes), name
    fields = re.search(r"typedef struct srgd_threshold_image \{(.*?)\}", flat, flags=re.S).group(1)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert names == [f[0] for f in TH.ThresholdImage._fields_] and C.sizeof(TH.ThresholdImage) == 48
    assert os.path.exists(TH.LIB_PATH), "build the library first (python -m srgd_amd.build)"
    assert _exports(TH.LIB_PATH) == ENTRIES
    # the engine's export table is what it was, and no other library holds a threshold name
    assert _exports(_lib.LIB_PATH) == set(_lib.PROTOTYPES)
    for mod in (_lib, GD, SV):
        assert not any("threshold" in n for n in _exports(mod.LIB_PATH)), mod.__name__
        assert not set(TH.PROTOTYPES) & set(mod.PROTOTYPES)
    text = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("key(v) is the bit pattern of v with the sign bit cleared, compared as uint32", "NaNs sort last",
                   "pos = (double)q * (double)(n - 1);  lo = floor(pos);  hi = min(lo + 1, n - 1);  frac = (float)(pos - lo)",
                   "s_raw = a_lo + frac * (a_hi - a_lo)", "s = (s_raw < 1) ? 1 : s_raw, so a NaN s_raw stays NaN",
                   "t = v < -s ? -s : (v > s ? s : v);  y = t / s (IEEE division);  d = y - v;  x_start = y;",
                   "if d != 0: img = img + weight_img * d", "Everything outside the update boxes keeps its bytes",
                   "A non-finite s has no special case", "bit-identical to the call on that image alone",
                   "No floating-point atomics anywhere", "Asynchronous on `stream`; no allocation, no synchronisation"):
        assert phrase in text, phrase
    source = open(os.path.join(ROOT, "srgd_amd", "csrc", "threshold.hip")).read()
    assert "asm" not in source and "hipMalloc" not in source and "Synchronize" not in source
    assert not re.search(r"atomicAdd\([^;]*(float|f32)", source) and "atomicAdd(&mine[i], cnt)" in source
    build = open(os.path.join(ROOT, "srgd_amd", "build.py")).read()
    assert '"threshold.hip": ["-ffp-contract=off"]' in build and "srgd_threshold*" in build


def test_the_step_scalars_keep_their_layout_and_the_schedule_sets_the_switch():
    assert [f[0] for f in _lib.StepScalars._fields_][-1] == "no_clamp" and C.sizeof(_lib.StepScalars) == 32
    assert _lib.StepScalars.no_clamp.offset == 28 and _lib.StepScalars.no_clamp.size == 4
    header = open(os.path.join(ROOT, "include", "srgd_hip.h")).read()
    record = re.search(r"typedef struct srgd_step_scalars \{(.*?)\} srgd_step_scalars;", header, flags=re.S).group(1)
    assert "float no_clamp;" in record and "reserved" not in record
    kernels = open(os.path.join(ROOT, "srgd_amd", "csrc", "kernels.hpp")).read()
    assert re.search(r"float sigma_next;[^\n]*\n\s*float no_clamp;", kernels)
    assert "if (sc.no_clamp == 0.0f) x0 = clamp_keep_nan(x0, -1.0f, 1.0f);" in open(os.path.join(ROOT, "srgd_amd", "csrc", "sampler.hip")).read()
    plain, levels = MODEL._schedule(5)
    assert all(s.no_clamp == 0.0 for s in plain)
    for solver in (None, ("ddim", 0.5, "logsnr"), ("dpmpp2m", None, "logsnr")):
        base, lv0 = MODEL._schedule(5, *(solver or ()))
        free, lv1 = MODEL._schedule_of(5, solver, no_clamp=True)
        assert lv0 == lv1 and all(s.no_clamp == 1.0 for s in free)
        for a, b in zip(base, free):                     # nothing else moves
            assert bytes(a)[:28] == bytes(b)[:28] and bytes(a)[28:] == b"\0\0\0\0"
        for kw in (dict(), dict(no_clamp=False)):
            same, lv1 = MODEL._schedule_of(5, solver, **kw)
            assert lv0 == lv1 and [bytes(a) for a in same] == [bytes(a) for a in base]
    assert list(inspect.signature(MODEL._schedule_of).parameters) == ["num_sample_steps", "solver", "no_clamp"]


def test_refusals_need_no_gpu():
    # every refusal is decided on the host before anything is launched, so it can be checked here: -1 and a message
    lib = TH.lib()
    at = lambda v: C.c_void_p(v)                           # noqa: E731
    # never dereferenced: a refused call launches nothing.  A 20 x 20 box in a 256 x 256 canvas: 786,432 bytes of canvas
    img, xs, out, scr = 1 << 24, 2 << 24, 3 << 24, 4 << 24

    def rec(**kw):
        base = dict(canvas_off=0, Hp=256, Wp=256, top=118, left=118, H=20, W=20, box_t=100, box_l=110, box_h=60, box_w=40)
        return TH.ThresholdImage(**dict(base, **kw))

    def call(images=None, n=None, **kw):
        images = [rec()] if images is None else images
        a = dict(dict(img=at(img), xs=at(xs), out=at(out), scr=at(scr), q=0.995, w=0.5), **kw)
        arr = (TH.ThresholdImage * len(images))(*images) if images != "null" else None
        rc = lib.srgd_threshold_step(a["img"], a["xs"], arr, len(images) if n is None else n, a["q"], a["w"], a["out"], a["scr"], None)
        return rc, lib.srgd_threshold_last_error().decode()
    canvas = 4 * 3 * 256 * 256
    cases = {"null": [dict(img=None), dict(xs=None), dict(out=None), dict(scr=None), dict(images="null", n=1)],
             "n_images": [dict(n=0), dict(n=-1)],
             "q must be in (0, 1]": [dict(q=0.0), dict(q=-0.5), dict(q=1.0000001), dict(q=float("nan")), dict(q=float("inf"))],
             "finite": [dict(w=float("nan")), dict(w=float("inf")), dict(w=float("-inf"))],
             "bad size": [dict(images=[rec(H=0)]), dict(images=[rec(W=0)]), dict(images=[rec(H=-2)]), dict(images=[rec(), rec(canvas_off=3 * 65536, W=0)])],
             "bad canvas": [dict(images=[rec(Hp=0)]), dict(images=[rec(Wp=-1)]),
                            dict(images=[rec(Hp=26755, Wp=26755)])],
             "update box": [dict(images=[rec(box_t=-1)]), dict(images=[rec(box_l=-1)]), dict(images=[rec(box_t=100, box_h=157)]),
                            dict(images=[rec(box_l=110, box_w=147)]), dict(images=[rec(box_h=0)]), dict(images=[rec(Wp=149)])],
             "statistics box": [dict(images=[rec(top=99)]), dict(images=[rec(left=109)]), dict(images=[rec(H=43)]), dict(images=[rec(W=33)]),
                                dict(images=[rec(top=141)]), dict(images=[rec(box_t=119)])],
             "offset outside": [dict(images=[rec(canvas_off=-1)]), dict(images=[rec(canvas_off=1 << 40)])],
             "4-byte aligned": [dict(img=at(img + 2)), dict(xs=at(xs + 1)), dict(out=at(out + 3))],
             "256-byte aligned": [dict(scr=at(scr + 128)), dict(scr=at(scr + 16))],
             "overlapping canvases": [dict(images=[rec(), rec()]), dict(images=[rec(), rec(canvas_off=3 * 65536 - 1)]),
                                      dict(images=[rec(canvas_off=3 * 65536), rec(), rec(canvas_off=6 * 65536 - 7)])],
             "overlapping buffers": [dict(xs=at(img)), dict(xs=at(img + canvas - 4)), dict(xs=at(img - canvas + 4)), dict(out=at(img + 4)),
                                     dict(out=at(xs + canvas - 4)), dict(scr=at(img)), dict(scr=at(xs + 256)), dict(scr=at(out)),
                                     dict(out=at(scr + 8448 - 4))]}
    for word, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == -1 and word in msg and msg.startswith("srgd_threshold_step: "), (kw, msg)
    assert 3 * 26755 * 26755 >= 2 ** 31 > 3 * 26754 * 26754
    assert TH.scratch_bytes(1) == 8448 and TH.scratch_bytes(130) == 130 * 8448 and 8448 % 256 == 0
    assert lib.srgd_threshold_scratch_bytes(0) == 0 and lib.srgd_threshold_scratch_bytes(-4) == 0


def test_host_side_checks_of_the_module():
    assert TH.check_percentile(None) is None and TH.check_percentile(0) is None and TH.check_percentile(0.0) is None
    assert TH.check_percentile(1) == 1.0 and TH.check_percentile(0.995) == float(np.float32(0.995)) != 0.995
    assert TH.check_percentile(1.00000001) == 1.0                        # its fp32 rounding lies in (0, 1]
    for bad in (-0.1, 1.5, 1.0000001, float("nan"), float("inf"), "1", True, [0.5], 1e-60):
        with pytest.raises(ValueError, match="percentile"):
            TH.check_percentile(bad)
    recs = TH.records([TC.NESTED, (4096, 768, 768, 234, 234, 300, 300, 128, 128, 512, 512)])
    assert [getattr(recs[1], f[0]) for f in TH.ThresholdImage._fields_] == [4096, 768, 768, 234, 234, 300, 300, 128, 128, 512, 512]
    for bad in ([], [(-1,) + TC.NESTED[1:]], [TC.NESTED[:3] + (1,) + TC.NESTED[4:]], [TC.NESTED[:5] + (8,) + TC.NESTED[6:]],
                [TC.NESTED[:9] + (12, 11)], [TC.NESTED[:6] + (0,) + TC.NESTED[7:]], [(0, 26755, 26755, 0, 0, 4, 4, 0, 0, 4, 4)]):
        with pytest.raises(ValueError, match="dynamic_threshold"):
            TH.records(bad)
    for bad in (0, -1, True, 1.0, None):
        with pytest.raises(ValueError, match="n_images"):
            TH.scratch_bytes(bad)
    f32 = lambda n: torch.zeros(n, dtype=torch.float32)                       # noqa: E731
    recs = TH.records([(0, 13, 16) + TC.NESTED[3:]])
    ok = dict(img=f32(624), x_start=f32(624), recs=recs, q=0.9, weight_img=0.5, s_out=f32(1), scratch=torch.zeros(8448, dtype=torch.uint8))
    for kw in (dict(q="1"), dict(weight_img=None), dict(recs=[recs[0]]), dict(recs=None), dict(img=f32(624).double()), dict(x_start=f32(623)),
               dict(s_out=f32(0)), dict(s_out=f32(1).double()), dict(scratch=torch.zeros(8447, dtype=torch.uint8)), dict(scratch=f32(8448))):
        with pytest.raises(ValueError, match="dynamic_threshold"):
            TH.threshold_step_flat(**dict(ok, **kw))
    with pytest.raises(_lib.SrgdHipError, match="no CPU fallback"):          # a missing GPU is an error, never another path
        TH.threshold_step_flat(**ok)
    assert list(inspect.signature(TH.threshold_step_flat).parameters) == ["img", "x_start", "recs", "q", "weight_img", "s_out", "scratch"]
    source = inspect.getsource(TH)
    assert "torch.empty" not in source and "torch.zeros" not in source and ".clone(" not in source      # the caller owns every buffer


def test_the_new_kernels_and_the_step_kernel_do_not_spill_and_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_table
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "threshold.hip"), ["-ffp-contract=off"]) if "threshold_" in r["name"]]
    assert sorted(r["name"] for r in rows) == ["threshold_apply_kernel", "threshold_hist_kernel", "threshold_scan_kernel"]
    for r in rows:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["lds"] <= 160 * 1024 // 8 and r["vgpr"] <= 64, r         # eight 256-thread workgroups per CU
    lds = {r["name"]: r["lds"] for r in rows}
    assert lds["threshold_hist_kernel"] == 4 * 2048 and lds["threshold_scan_kernel"] == 4 * (2048 + 256 + 4) and lds["threshold_apply_kernel"] == 0
    step = [r for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "sampler.hip")) if "final_step_kernel" in r["name"]]
    assert len(step) >= 2
    for r in step:
        assert r["spill"] == 0 and r["scratch"] == 0 and 0 < r["vgpr"] <= 128, r


# ------------------------------------------------------------------------------------------- the flag and the keywords
def test_the_flag_parses():
    assert INF.parse_args(_argv()).dynamic_threshold == 0.0
    assert INF.parse_args(_argv("--dynamic_threshold", "0.995")).dynamic_threshold == 0.995
    args = INF.parse_args(_argv("--dynamic_threshold", "1", "--sampler", "dpmpp2m", "--step_spacing", "logsnr", "--consistency_guidance", "0.5"))
    assert args.dynamic_threshold == 1.0 and args.sampler == "dpmpp2m" and args.consistency_guidance == 0.5
    for bad in ("-0.1", "1.01", "nan", "inf"):
        with pytest.raises(SystemExit, match="--dynamic_threshold"):
            INF.parse_args(_argv("--dynamic_threshold", bad))
    with pytest.raises(SystemExit):
        INF.parse_args(_argv("--dynamic_threshold", "high"))


def test_the_keyword_defaults_to_off_and_the_untiled_sample_has_none():
    ddpm, edm = MODEL.ConditionalContinuousTimeGaussianDiffusionSR, MODEL.ConditionalElucidatedDiffusionSR
    for fn in (INF.sr_target_image, INF.sr_target_images, INF.sr_target_images_mixed, INF.sr_target_images_seeded, ddpm.tiled_sample,
               edm.tiled_sample):
        assert inspect.signature(fn).parameters["dynamic_threshold"].default is None, fn.__qualname__
    assert inspect.signature(INF.batch_sr_target_images).parameters["dynamic_threshold"].default == 0.0
    assert inspect.signature(ddpm.tiled_sample).parameters["threshold_log"].default is None
    for fn in (ddpm.sample, edm.sample, edm.sample_org, edm.sample_using_dpmpp):
        assert "dynamic_threshold" not in inspect.signature(fn).parameters, fn.__qualname__
    assert INF._threshold_kw(0.0) == {} and INF._threshold_kw(None) == {} and INF._threshold_kw(0) == {}
    assert INF._threshold_kw(0.995) == {"dynamic_threshold": 0.995}


class _Unused:
    """A sampler whose every attribute access fails the test: ``tiled_sample`` must refuse before it touches the model."""
    canvas_group = None

    def __getattr__(self, name):
        raise AssertionError(f"the sampler was touched ({name}) before the arguments were checked")


class _Sharded(_Unused):
    canvas_group = object()


def test_the_wrappers_check_the_percentile_on_entry_and_refuse_what_is_not_built():
    fn = inspect.unwrap(MODEL.ConditionalContinuousTimeGaussianDiffusionSR.tiled_sample)
    cond = torch.zeros(1, 3, 256, 256)
    for bad in (-0.5, 1.5, float("nan"), "1"):
        with pytest.raises(ValueError, match="percentile"):
            fn(_Unused(), condition_x=cond, dynamic_threshold=bad)
    with pytest.raises(ValueError, match="threshold_log"):
        fn(_Unused(), condition_x=cond, dynamic_threshold=0.9, threshold_log=())
    with pytest.raises(NotImplementedError, match="canvas_group"):
        fn(_Sharded(), condition_x=cond, dynamic_threshold=0.995)
    edm = inspect.unwrap(MODEL.ConditionalElucidatedDiffusionSR.tiled_sample)
    for p in (0.995, 1, 1.0):
        with pytest.raises(NotImplementedError, match="DDPM sampler only"):
            edm(_Unused(), condition_x=cond, dynamic_threshold=p)
    with pytest.raises(ValueError, match="percentile"):
        edm(_Unused(), condition_x=cond, dynamic_threshold=2.0)


def test_the_sr_functions_and_the_batch_loop_hand_the_keyword_on_only_when_it_is_set(tmp_path, monkeypatch):
    seen = []

    class Fake:
        device = torch.device("cpu")
        device_noise_seed = 0

        def tiled_sample(self, **kw):
            seen.append(kw)
            cond = kw["condition_x"]
            return [torch.zeros_like(c) for c in cond] if isinstance(cond, list) else torch.zeros_like(cond)
    monkeypatch.setattr(INF, "upsample_bicubic_on_device", lambda im, scale, dev: torch.zeros(1, 3, im.size[1] * scale, im.size[0] * scale))
    monkeypatch.setattr(INF, "unit_tensor_to_pil_on_device",
                        lambda t: Image.fromarray(np.zeros((t.shape[-2], t.shape[-1], 3), dtype=np.uint8), "RGB"))
    im = Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8), "RGB")
    runs = (lambda **kw: INF.sr_target_image(im, Fake(), **kw), lambda **kw: INF.sr_target_images([im, im], Fake(), **kw),
            lambda **kw: INF.sr_target_images_mixed([im, im], Fake(), **kw),
            lambda **kw: INF.sr_target_images_seeded([im, im], [1, 2], Fake(), **kw))
    for run in runs:
        seen.clear()
        run()
        run(dynamic_threshold=0.0)
        run(dynamic_threshold=None)
        assert len(seen) == 3 and all("dynamic_threshold" not in kw for kw in seen)
        run(dynamic_threshold=0.995)
        assert seen[3]["dynamic_threshold"] == 0.995 and set(seen[3]) - set(seen[0]) == {"dynamic_threshold"}
    # the batch loop
    calls = []

    def fake(kind):
        def run(images, *a, **kw):
            ims = images if isinstance(images, list) else [images]
            calls.append((kind, len(ims), dict(kw)))
            outs = [Image.fromarray(np.zeros((i_.size[1] * 4, i_.size[0] * 4, 3), dtype=np.uint8), "RGB") for i_ in ims]
            return outs if isinstance(images, list) else outs[0]
        return run
    for name, kind in (("sr_target_image", "solo"), ("sr_target_images", "same"), ("sr_target_images_mixed", "mixed"),
                       ("sr_target_images_seeded", "seeded")):
        monkeypatch.setattr(INF, name, fake(kind))
    indir = tmp_path / "in"
    indir.mkdir()
    for name, (w, h) in {"a": (64, 64), "b": (64, 64), "c": (48, 64)}.items():
        Image.fromarray(np.zeros((h, w, 3), dtype=np.uint8), "RGB").save(indir / f"{name}.png")
    for tag, kw in (("solo", {}), ("same", dict(lockstep=2)), ("mixed", dict(lockstep_tiles=8)), ("seeded", dict(samples=2))):
        calls.clear()
        INF.batch_sr_target_images(str(indir), str(tmp_path / (tag + "_off")), None, seed=71, **kw)
        INF.batch_sr_target_images(str(indir), str(tmp_path / (tag + "_zero")), None, seed=71, dynamic_threshold=0.0, **kw)
        assert calls and all("dynamic_threshold" not in c[2] for c in calls), tag
        kinds_off = [c[:2] for c in calls[:len(calls) // 2]]
        calls.clear()
        INF.batch_sr_target_images(str(indir), str(tmp_path / (tag + "_on")), None, seed=71, dynamic_threshold=0.995, **kw)
        assert [c[:2] for c in calls] == kinds_off and all(c[2]["dynamic_threshold"] == 0.995 for c in calls), tag
    with pytest.raises(ValueError, match="percentile"):
        INF.batch_sr_target_images(str(indir), str(tmp_path / "bad"), None, dynamic_threshold=1.5)
