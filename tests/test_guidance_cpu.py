"""LR-consistency guidance, host side (no GPU): the two yardsticks of tests/guidance_cases.py (U(D(const)) = const up to the rounding of
the coefficient integers; the restated loop with no guided step is the oracle's loop bit for bit; on the end-to-end cases of the GPU
tests the guided oracle lies closer to its input than the unguided one, so the GPU inequality is not vacuous), the library's
coefficient vectors against Pillow's rows, the C-ABI declarations, exports and refusals of the new library, the module's own checks,
the resource table of the two kernels, the flags, the keywords and the batch loop with fake samplers, and what is refused."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import pil_resample as PR
from oracle import srgd_oracle as O
from srgd_amd import _lib
from srgd_amd import backproject as BP
from srgd_amd import consistency as CS
from srgd_amd import ensemble as EN
from srgd_amd import guidance as GD
from srgd_amd import inference as INF
from srgd_amd import metrics as MX
from srgd_amd import model as MODEL
from tests import guidance_cases as G
from tests.lib_exports import exports as _exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")
ENTRIES = {"srgd_guidance_step", "srgd_guidance_coeffs", "srgd_guidance_last_error"}
KEYWORDS = ("consistency_guidance", "consistency_guidance_start_steps")


def _argv(*extra):
    return ["-c", CONF, "-m", "ckpt.pth", "--input_dir", "in", "--output_dir", "out", *extra]


# ------------------------------------------------------------------------------------------- yardstick (a)
@pytest.mark.parametrize("h,w", [(5, 5), (6, 7), (16, 23), (65, 70)])
def test_a_constant_is_reduced_and_enlarged_to_itself(h, w):
    # the integers of a row sum to 2^22 - 1, 2^22 or 2^22 + 1 (the taps are rounded one by one), so a row of the operator sums to 1
    # within 2^-22 and four passes keep a constant within 4 * 2^-22 of itself
    for n in (h, w):
        down, up = G.matrices(n)
        assert set(np.rint((down.sum(axis=1) - 1) * 2 ** 22).astype(int)) <= {-1, 0, 1}
        assert set(np.rint((up.sum(axis=1) - 1) * 2 ** 22).astype(int)) <= {-1, 0, 1}
        assert np.abs(down).sum(axis=1).max() <= 1.4 and np.abs(up).sum(axis=1).max() <= 1.4       # the sum|k| of the fp32 bar
    for a in (1.0, -0.75, 0.3):
        got = G.ud64(np.full((3, 4 * h, 4 * w), a))
        assert got.shape == (3, 4 * h, 4 * w)
        assert np.abs(got - a).max() <= 4 * 2.0 ** -22 * abs(a) * 1.001
    # D alone is the reduction the consistency yardstick measures with, up to its 8-bit roundings (half a level per pass, amplified by
    # the vertical pass's sum|k| < 1.2, and the final rounding)
    out, _ = G.K.random_pair(h, w, 3)
    want = G.K.pillow_down(out).astype(np.float64)
    inner = G.d64(out.transpose(2, 0, 1).astype(np.float64)).transpose(1, 2, 0)
    assert np.abs(np.clip(inner, 0, 255) - want).max() <= 0.5 * 1.2 + 0.5 + 1e-9
    # U alone against Pillow's enlargement of the same rounded image
    up_pil = G.K.pillow_up(G.K.pillow_down(out)).astype(np.float64)
    assert np.abs(np.clip(G.u64(want.transpose(2, 0, 1)).transpose(1, 2, 0), 0, 255) - up_pil).max() <= 0.5 * 1.24 + 0.5 + 1e-9


def test_the_footprint_of_one_element_is_sixteen_pixels():
    # the GPU's non-finite test leaves 24 pixels around a NaN: U(D(.)) spreads an element no farther than 16 along either axis
    for n, p in ((12, 0), (12, 23), (12, 47), (12, 20), (5, 9)):
        down, up = G.matrices(n)
        reach = np.nonzero((up @ down)[:, p])[0]
        assert p in reach and np.abs(reach - p).max() <= 16, (n, p, reach)


# ------------------------------------------------------------------------------------------- yardstick (b)
def _oracle_args(name, steps=None):
    case = G.E2E_CASES[name]
    _, cond = G.e2e_input(name)
    return case, cond, dict(batch_size=case["batch_size"], num_sample_steps=steps or case["steps"])


@pytest.mark.parametrize("name,steps", [("tile256", 6), ("geo300", 2)])
def test_the_restated_loop_without_a_guided_step_is_the_oracles_loop(name, steps):
    case, cond, kw = _oracle_args(name, steps)
    sd, cfg, label = O.strip_model_prefix(G.state_dict()), O.UnetCfg(dim=G.DIM), torch.tensor([G.LABEL])
    with torch.inference_mode():
        torch.manual_seed(case["seed"])
        want = O.tiled_sample(sd, cfg, cond, label, **kw)
        for extra in (dict(consistency_guidance=0.0), dict(consistency_guidance=1.0, consistency_guidance_start_steps=steps)):
            torch.manual_seed(case["seed"])
            trace = {}
            got = G.guided_tiled_sample(sd, cfg, cond, label, trace=trace, **kw, **extra)
            assert torch.equal(got, want), extra
            assert len(trace["img"]) == len(trace["x_start"]) == steps
        torch.manual_seed(case["seed"])
        moved = G.guided_tiled_sample(sd, cfg, cond, label, consistency_guidance=1.0, consistency_guidance_start_steps=steps - 1, **kw)
    assert not torch.equal(moved, want)                      # guiding the last step alone already moves the output


@pytest.mark.parametrize("name", list(G.E2E_CASES))
def test_on_the_end_to_end_cases_the_guided_oracle_lies_closer_to_its_input(name):
    lr, cond = G.e2e_input(name)
    assert cond.shape == (1, 3, 4 * lr.shape[0], 4 * lr.shape[1]) and float(cond.min()) >= 0 and float(cond.max()) <= 1
    guided, trace = G.e2e_oracle(name, True)
    plain, _ = G.e2e_oracle(name, False)
    assert len(trace["img"]) == G.E2E_CASES[name]["steps"]
    a, b = G.lr_mse(guided, lr), G.lr_mse(plain, lr)
    print(f"{name}: LR-MSE of the oracle guided {a:.2f}, unguided {b:.2f}")
    assert a < b, (a, b)


# ------------------------------------------------------------------------------------------- coefficients
def test_the_librarys_vectors_are_pillows_rows_over_two_to_the_22():
    down, up = GD.coeffs()
    assert len(down) == 5 and all(len(v) == 16 for v in down) and len(up) == 16 and all(len(v) == 4 for v in up)
    for n in (5, 6, 37, 64):
        bounds, kk = PR.precompute_coeffs(4 * n, n)
        for i in range(n):
            v = 0 if i == 0 else 1 if i == 1 else 3 if i == n - 2 else 4 if i == n - 1 else 2
            frame = [0.0] * 16
            for t in range(int(bounds[i, 1])):
                frame[int(bounds[i, 0]) + t - (4 * i - 6)] = float(kk[i, t]) / 2 ** 22
            assert down[v] == frame, (n, i)
        bounds, kk = PR.precompute_coeffs(n, 4 * n)
        for j in range(4 * n):
            v = j if j < 6 else (10 + j - (4 * n - 6) if j >= 4 * n - 6 else 6 + (j - 6) % 4)
            frame = [0.0] * 4
            for t in range(int(bounds[j, 1])):
                frame[int(bounds[j, 0]) + t - ((j - 6) // 4)] = float(kk[j, t]) / 2 ** 22
            assert up[v] == frame, (n, j)
    # every coefficient is an integer of fewer than 24 bits over 2^22: exact in fp32
    assert all(float(np.float32(c)) == c and float(c * 2 ** 22).is_integer() and abs(c) < 2 for v in down + up for c in v)
    # the enlargement's vectors are the back-projection library's sixteen
    assert [[c for c in v if c != 0.0] for v in up] == [[k / 2 ** 22 for k in v if k != 0] for v in BP.coeffs()]
    lib = GD.lib()
    buf = ((C.c_float * 16) * 5)()
    assert lib.srgd_guidance_coeffs(None, C.cast(buf, C.c_void_p)) == -1 and lib.srgd_guidance_coeffs(C.cast(buf, C.c_void_p), None) == -1
    assert lib.srgd_guidance_last_error().decode().startswith("srgd_guidance_coeffs: ")


# ------------------------------------------------------------------------------------------- C ABI, refusals, resources
def test_entries_are_declared_prototyped_and_exported_by_a_library_of_their_own():
    header = open(os.path.join(ROOT, "include", "srgd_guidance.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(srgd_[a-z0-9_]+)\s*\(", flat))
    assert declared == ENTRIES == set(GD.PROTOTYPES)
    for name, (_, argtypes) in GD.PROTOTYPES.items():
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", flat).group(1).strip()
        assert (0 if params == "void" else len(params.split(","))) == len(argtypes), name
    # the record of the header is the ctypes structure
    fields = re.search(r"typedef struct srgd_guidance_image \{(.*?)\}", flat, flags=re.S).group(1)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert names == [f[0] for f in GD.GuidanceImage._fields_] and C.sizeof(GD.GuidanceImage) == 40
    assert os.path.exists(GD.LIB_PATH), "build the library first (python -m srgd_amd.build)"
    assert _exports(GD.LIB_PATH) == ENTRIES
    assert GD.lib().srgd_guidance_last_error() is not None                     # binds every prototype
    # the five other libraries: their exports are what their modules prototype, and none holds a guidance name
    for mod in (_lib, MX, EN, CS, BP):
        assert _exports(mod.LIB_PATH) == set(mod.PROTOTYPES), mod.__name__
        assert not any("guidance" in n for n in _exports(mod.LIB_PATH)), mod.__name__
        assert not set(GD.PROTOTYPES) & set(mod.PROTOTYPES)
    for phrase in ("C = 2 * cond01 - 1", "sum_t down[v(i)][t] * X[y][4i - 6 + t]", "No 8-bit rounding and no clipping in between or after",
                   "g = C - U(D(X));  x_start = fmaf(weight_x0, g, x_start);  img = fmaf(weight_img, g, img), inside the crop box only",
                   "Everything outside the crop boxes keeps its bytes", "There are no clamps",
                   "scratch: device memory owned by the caller, sum_i roundup(12*h_i*w_i, 256) bytes",
                   "bit-identical to the call on that image alone", "Asynchronous on `stream`; no allocation, no synchronisation"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", header), phrase


def test_refusals_need_no_gpu():
    # every refusal is decided on the host before anything is launched, so it can be checked here: -1 and a message
    lib = GD.lib()
    at = lambda v: C.c_void_p(v)                           # noqa: E731
    # never dereferenced: a refused call launches nothing.  A 5x5 image in a 256x256 canvas: 786,432 bytes of canvas, 4,800 of cond01
    img, xs, cond, scr = 1 << 24, 2 << 24, 3 << 24, 4 << 24

    def rec(**kw):
        base = dict(canvas_off=0, cond_off=0, Hp=256, Wp=256, top=118, left=118, h=5, w=5)
        return GD.GuidanceImage(**dict(base, **kw))

    def call(images=None, n=None, **kw):
        images = [rec()] if images is None else images
        a = dict(dict(img=at(img), xs=at(xs), cond=at(cond), scr=at(scr), w0=1.0, wi=0.5), **kw)
        arr = (GD.GuidanceImage * len(images))(*images) if images != "null" else None
        rc = lib.srgd_guidance_step(a["img"], a["xs"], a["cond"], arr, len(images) if n is None else n, a["w0"], a["wi"], a["scr"], None)
        return rc, lib.srgd_guidance_last_error().decode()
    canvas = 4 * 3 * 256 * 256
    cases = {"null": [dict(img=None), dict(xs=None), dict(cond=None), dict(scr=None), dict(images="null", n=1)],
             "n_images": [dict(n=0), dict(n=-1)],
             "bad size": [dict(images=[rec(h=4)]), dict(images=[rec(w=4)]), dict(images=[rec(h=0)]), dict(images=[rec(w=-3)]),
                          dict(images=[rec(), rec(canvas_off=3 * 65536, w=4)])],
             "bad canvas": [dict(images=[rec(Hp=0)]), dict(images=[rec(Wp=-1)]), dict(images=[rec(Hp=26755, Wp=26755, top=0, left=0)])],
             "crop box": [dict(images=[rec(top=-1)]), dict(images=[rec(left=-1)]), dict(images=[rec(top=237)]), dict(images=[rec(left=237)]),
                          dict(images=[rec(h=65)]), dict(images=[rec(Wp=137)])],
             "offset outside": [dict(images=[rec(canvas_off=-1)]), dict(images=[rec(cond_off=-4)]), dict(images=[rec(canvas_off=1 << 40)])],
             "finite": [dict(w0=float("nan")), dict(wi=float("inf")), dict(w0=float("-inf")), dict(wi=float("nan"))],
             "4-byte aligned": [dict(img=at(img + 2)), dict(xs=at(xs + 1)), dict(cond=at(cond + 3))],
             "256-byte aligned": [dict(scr=at(scr + 128)), dict(scr=at(scr + 16))],
             "overlapping canvases": [dict(images=[rec(), rec()]), dict(images=[rec(), rec(canvas_off=3 * 65536 - 1)]),
                                      dict(images=[rec(canvas_off=3 * 65536), rec(), rec(canvas_off=6 * 65536 - 7)])],
             "overlapping buffers": [dict(xs=at(img)), dict(xs=at(img + canvas - 4)), dict(xs=at(img - canvas + 4)), dict(cond=at(img + 4)),
                                     dict(cond=at(xs + canvas - 4)), dict(scr=at(img)), dict(scr=at(xs + 256)), dict(scr=at(cond)),
                                     dict(cond=at(scr + 256 - 4))]}
    for word, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == -1 and word in msg and msg.startswith("srgd_guidance_step: "), (kw, msg)
    assert 3 * 26755 * 26755 >= 2 ** 31 > 3 * 26754 * 26754
    # disjoint is enough: buffers that touch are taken (the call would launch, so it is not made here) - the refusals above are strict
    assert canvas == 786432 and GD.scratch_bytes([(5, 5)]) == 512


def test_host_side_checks_of_the_module():
    assert (GD.MIN_SIDE, GD.SCALE, GD.ALIGN) == (5, 4, 256)
    # the header's scratch formula: D of 12hw bytes per image, rounded up to 256
    assert GD.scratch_bytes([(5, 5)]) == 512 and GD.scratch_bytes([(16, 16)]) == 3072
    assert GD.scratch_bytes([(65, 70), (5, 5)]) == 54784 + 512 and 12 * 65 * 70 == 54600
    with pytest.raises(ValueError, match="size"):
        GD.scratch_bytes([(4, 40)])
    assert GD.check_weight(None) is None and GD.check_weight(0) is None and GD.check_weight(0.0) is None
    assert GD.check_weight(1) == 1.0 and GD.check_weight(0.25) == 0.25
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "1", True, [1.0]):
        with pytest.raises(ValueError, match="weight"):
            GD.check_weight(bad)
    assert GD.check_start_steps(0) == 0 and GD.check_start_steps(7) == 7
    for bad in (-1, 1.0, "2", True, None):
        with pytest.raises(ValueError, match="start_steps"):
            GD.check_start_steps(bad)
    assert GD.check_hr_sizes([(20, 28), (1024, 1024)]) == [(5, 7), (256, 256)]
    for bad in ((16, 40), (40, 16), (22, 40), (40, 41), (300, 302)):
        with pytest.raises(ValueError, match="bad image size"):
            GD.check_hr_sizes([(20, 20), bad])
    recs, low = GD.records([(0, 0, 256, 256, 118, 118, 20, 20), (3 * 65536, 1200, 768, 768, 254, 244, 260, 280)])
    assert low == [(5, 5), (65, 70)] and len(recs) == 2
    assert (recs[1].canvas_off, recs[1].cond_off, recs[1].Hp, recs[1].Wp, recs[1].top, recs[1].left, recs[1].h, recs[1].w) == \
        (196608, 1200, 768, 768, 254, 244, 65, 70)
    for bad in ([], [(0, 0, 256, 256, 118, 118, 16, 20)], [(0, 0, 256, 256, 240, 118, 20, 20)], [(0, 0, 256, 256, 118, -1, 20, 20)],
                [(-1, 0, 256, 256, 118, 118, 20, 20)], [(0, -1, 256, 256, 118, 118, 20, 20)], [(0, 0, 26755, 26755, 0, 0, 20, 20)]):
        with pytest.raises(ValueError, match="consistency_guidance"):
            GD.records(bad)
    f32 = lambda n: torch.zeros(n, dtype=torch.float32)                       # noqa: E731
    recs, _ = GD.records([(0, 0, 256, 256, 118, 118, 20, 20)])
    ok = dict(img=f32(3 * 65536), x_start=f32(3 * 65536), cond01=f32(1200), recs=recs, weight_x0=1.0, weight_img=0.5,
              scratch=torch.zeros(512, dtype=torch.uint8))
    for kw in (dict(weight_x0=float("nan")), dict(weight_img=float("inf")), dict(weight_x0="1"), dict(recs=[recs[0]]), dict(recs=None),
               dict(img=f32(3 * 65536).double()), dict(x_start=f32(3 * 65536 - 1)), dict(cond01=f32(1199)), dict(img=f32(10)),
               dict(scratch=torch.zeros(511, dtype=torch.uint8)), dict(scratch=f32(512)), dict(cond01=None)):
        with pytest.raises(ValueError, match="consistency_guidance"):
            GD.guide_step_flat(**dict(ok, **kw))
    with pytest.raises(_lib.SrgdHipError, match="no CPU fallback"):          # a missing GPU is an error, never another path
        GD.guide_step_flat(**ok)
    assert list(inspect.signature(GD.guide_step_flat).parameters) == ["img", "x_start", "cond01", "recs", "weight_x0", "weight_img", "scratch"]
    source = inspect.getsource(GD)
    assert "torch.empty" not in source and "torch.zeros" not in source and ".clone(" not in source      # the caller owns every buffer


def test_guidance_kernels_do_not_spill_and_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_table
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "guidance.hip")) if "guidance_" in r["name"]]
    assert sorted(r["name"] for r in rows) == ["guidance_reduce_kernel", "guidance_update_kernel"]
    for r in rows:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["lds"] <= 160 * 1024 // 3 and r["vgpr"] <= 128, r       # three 256-thread workgroups per CU and more
    lds = {r["name"]: r["lds"] for r in rows}
    assert lds["guidance_reduce_kernel"] == 4 * (72 * 144 + 72 * 32) + 320
    assert lds["guidance_update_kernel"] == 4 * (19 * 36 + 19 * 128) + 256


# ------------------------------------------------------------------------------------------- flags and keywords
def test_the_flags_parse():
    args = INF.parse_args(_argv())
    assert args.consistency_guidance == 0.0 and args.consistency_guidance_start_steps == 0
    args = INF.parse_args(_argv("--consistency_guidance", "0.5", "--consistency_guidance_start_steps", "3"))
    assert args.consistency_guidance == 0.5 and args.consistency_guidance_start_steps == 3
    args = INF.parse_args(_argv("--consistency_guidance", "1", "--consistency", "--back_project", "2", "--samples", "3", "--ensemble",
                                "--color_fix", "wavelet", "--lockstep", "2"))
    assert args.consistency_guidance == 1.0 and args.consistency is True and args.back_project == 2 and args.color_fix == "wavelet"
    for bad in ("-0.1", "1.01", "nan", "inf"):
        with pytest.raises(SystemExit, match="--consistency_guidance"):
            INF.parse_args(_argv("--consistency_guidance", bad))
    with pytest.raises(SystemExit, match="--consistency_guidance_start_steps"):
        INF.parse_args(_argv("--consistency_guidance", "1", "--consistency_guidance_start_steps", "-1"))
    with pytest.raises(SystemExit):
        INF.parse_args(_argv("--consistency_guidance", "much"))


def test_every_keyword_defaults_to_off_and_the_untiled_sample_has_none():
    ddpm, edm = MODEL.ConditionalContinuousTimeGaussianDiffusionSR, MODEL.ConditionalElucidatedDiffusionSR
    for fn in (INF.sr_target_image, INF.sr_target_images, INF.sr_target_images_mixed, INF.sr_target_images_seeded,
               INF.batch_sr_target_images, ddpm.tiled_sample, edm.tiled_sample):
        params = inspect.signature(fn).parameters
        assert params["consistency_guidance"].default == 0.0 and params["consistency_guidance_start_steps"].default == 0, fn.__qualname__
    for fn in (ddpm.sample, edm.sample, edm.sample_org, edm.sample_using_dpmpp):
        assert not set(KEYWORDS) & set(inspect.signature(fn).parameters), fn.__qualname__
    assert INF._guidance_kw(0.0) == {} and INF._guidance_kw(None) == {} and INF._guidance_kw(0, 5) == {}
    assert INF._guidance_kw(0.5, 2) == {"consistency_guidance": 0.5, "consistency_guidance_start_steps": 2}


class _Unused:
    """A sampler whose every attribute access fails the test: ``tiled_sample`` must refuse before it touches the model."""
    canvas_group = None

    def __getattr__(self, name):
        raise AssertionError(f"the sampler was touched ({name}) before the arguments were checked")


class _Sharded(_Unused):
    canvas_group = object()


def test_the_ddpm_wrapper_checks_the_keywords_and_the_sizes_on_entry():
    fn = inspect.unwrap(MODEL.ConditionalContinuousTimeGaussianDiffusionSR.tiled_sample)
    for bad in (-0.5, 1.5, float("nan"), "1"):
        with pytest.raises(ValueError, match="weight"):
            fn(_Unused(), condition_x=torch.zeros(1, 3, 256, 256), consistency_guidance=bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="start_steps"):
            fn(_Unused(), condition_x=torch.zeros(1, 3, 256, 256), consistency_guidance=1.0, consistency_guidance_start_steps=bad)
    for shape in ((1, 3, 300, 302), (2, 3, 16, 64), (1, 3, 258, 256)):
        with pytest.raises(ValueError, match="bad image size"):
            fn(_Unused(), condition_x=torch.zeros(*shape), consistency_guidance=1.0)
    with pytest.raises(ValueError, match="bad image size"):
        fn(_Unused(), condition_x=[torch.zeros(1, 3, 256, 256), torch.zeros(1, 3, 64, 30)], consistency_guidance=0.5)


def test_a_sharded_canvas_and_the_edm_wrapper_refuse_a_weight():
    fn = inspect.unwrap(MODEL.ConditionalContinuousTimeGaussianDiffusionSR.tiled_sample)
    with pytest.raises(NotImplementedError, match="canvas_group"):
        fn(_Sharded(), condition_x=torch.zeros(1, 3, 256, 256), consistency_guidance=0.5)
    edm = inspect.unwrap(MODEL.ConditionalElucidatedDiffusionSR.tiled_sample)
    for weight in (0.5, 1, 1.0):
        with pytest.raises(NotImplementedError, match="DDPM sampler only"):
            edm(_Unused(), condition_x=torch.zeros(1, 3, 256, 256), consistency_guidance=weight)
    with pytest.raises(ValueError, match="weight"):
        edm(_Unused(), condition_x=torch.zeros(1, 3, 256, 256), consistency_guidance=2.0)


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


def _inputs(tmp_path, sizes):
    indir = tmp_path / "in"
    indir.mkdir()
    rng = np.random.default_rng(0)
    for name, (w, h) in sizes.items():
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(indir / f"{name}.png")
    return indir


def test_the_batch_loop_hands_the_keywords_on_only_when_the_weight_is_set(tmp_path, monkeypatch):
    calls = []
    _fake_samplers(monkeypatch, calls)
    indir = _inputs(tmp_path, {"a": (64, 64), "b": (64, 64), "c": (48, 64)})
    run = lambda tag, **kw: INF.batch_sr_target_images(str(indir), str(tmp_path / tag), None, seed=71, **kw)  # noqa: E731
    for tag, kw in (("solo", {}), ("same", dict(lockstep=2)), ("mixed", dict(lockstep_tiles=8)), ("seeded", dict(samples=2))):
        calls.clear()
        run(tag + "_off", **kw)
        run(tag + "_zero", consistency_guidance=0.0, consistency_guidance_start_steps=4, **kw)
        assert calls and all(not set(KEYWORDS) & set(c[2]) for c in calls), tag
        kinds_off = [c[:2] for c in calls[:len(calls) // 2]]
        calls.clear()
        run(tag + "_on", consistency_guidance=0.5, consistency_guidance_start_steps=4, back_project=2, **kw)
        assert [c[:2] for c in calls] == kinds_off, tag
        assert all(c[2]["consistency_guidance"] == 0.5 and c[2]["consistency_guidance_start_steps"] == 4 and c[2]["back_project"] == 2
                   for c in calls), tag
        assert sorted(os.listdir(tmp_path / (tag + "_on"))) == sorted(os.listdir(tmp_path / (tag + "_off")))


def test_a_small_input_is_an_error_when_the_weight_is_set(tmp_path, monkeypatch):
    calls = []
    _fake_samplers(monkeypatch, calls)
    indir = _inputs(tmp_path, {"a": (64, 64), "tiny": (4, 9)})
    with pytest.raises(ValueError, match="tiny.png is 4x9"):
        INF.batch_sr_target_images(str(indir), str(tmp_path / "on"), None, consistency_guidance=1.0)
    assert not calls                                            # before anything is sampled
    INF.batch_sr_target_images(str(indir), str(tmp_path / "off"), None)
    assert len(calls) == 2


def test_the_sr_functions_hand_the_keywords_to_tiled_sample_only_when_the_weight_is_set(monkeypatch):
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
        run(consistency_guidance=0.0, consistency_guidance_start_steps=3)
        assert len(seen) == 2 and all(not set(KEYWORDS) & set(kw) for kw in seen)
        run(consistency_guidance=0.75, consistency_guidance_start_steps=3)
        assert seen[2]["consistency_guidance"] == 0.75 and seen[2]["consistency_guidance_start_steps"] == 3
        assert set(seen[2]) - set(seen[0]) == set(KEYWORDS)
