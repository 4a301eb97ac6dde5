"""The few-step samplers, host side (no GPU): the step tables against an independent float64 statement and against the parent
commit's default table, the order of the solvers on a case with a closed form, the restated loop of tests/solver_cases.py against the
oracle's own, the C-ABI declarations, exports and refusals of the new library, the module's own checks, the resource table of the
kernel, the flags, the keywords and the batch loop with fake samplers, and what is refused."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import srgd_oracle as O
from srgd_amd import _lib
from srgd_amd import backproject as BP
from srgd_amd import consistency as CS
from srgd_amd import ensemble as EN
from srgd_amd import guidance as GD
from srgd_amd import inference as INF
from srgd_amd import metrics as MX
from srgd_amd import model as MODEL
from srgd_amd import solver as SV
from tests import guidance_cases as G
from tests import solver_cases as SC
from tests.lib_exports import exports as _exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf", "conditional_continuous_linear_df8kost_dim128.yaml")
ENTRIES = {"srgd_solver_history_step", "srgd_solver_last_error"}
KEYWORDS = ("sampler", "eta", "step_spacing")
FIELDS = ("alpha", "sigma", "alpha_next", "c", "one_minus_c", "noise_scale", "sigma_next")
# _schedule(4) of the parent commit: the fields above per step, and the log-SNR list
PARENT_N4 = [
    (0.006737610790878534, 0.9999772906303406, 0.060051653534173965, 0.9874566793441772, 0.012543320655822754, 0.991915225982666,
     0.9981952905654907),
    (0.060051653534173965, 0.9981952905654907, 0.2864904999732971, 0.9595233201980591, 0.04047667980194092, 0.9384927749633789,
     0.9580830335617065),
    (0.2864904999732971, 0.9580830335617065, 0.731579065322876, 0.9223484396934509, 0.07765156030654907, 0.6547520756721497,
     0.6817566156387329),
    (0.731579065322876, 0.6817566156387329, 0.9999499917030334, 0.999884843826294, 0.00011515617370605469, 0.009999176487326622,
     0.009999752044677734)]
PARENT_N4_LOG_SNRS = [-10.000054359436035, -5.621487617492676, -2.4144582748413086, 0.14106504619121552]


def _argv(*extra):
    return ["-c", CONF, "-m", "ckpt.pth", "--input_dir", "in", "--output_dir", "out", *extra]


def _abs_table(scalars):
    """(A, B, S) the step kernel computes with from a ``StepScalars`` list, float64."""
    return [(s.alpha_next * s.one_minus_c / s.alpha, s.alpha_next * s.c, s.noise_scale) for s in scalars]


# ------------------------------------------------------------------------------------------- (a) the tables
def test_the_default_schedule_is_the_parent_commits_field_for_field():
    for call in (lambda: MODEL._schedule(4), lambda: MODEL._schedule(4, "ddpm", None, "time"),
                 lambda: MODEL._schedule(4, sampler="ddpm", step_spacing="time")):
        scalars, log_snrs = call()
        assert [tuple(getattr(s, f) for f in FIELDS) for s in scalars] == PARENT_N4
        assert log_snrs == PARENT_N4_LOG_SNRS
    assert list(inspect.signature(MODEL._schedule).parameters) == ["num_steps", "sampler", "eta", "step_spacing"]


@pytest.mark.parametrize("n", [4, 50])
def test_ddim_with_eta_one_is_the_ddpm_table_in_float64(n):
    for spacing in ("time", "logsnr"):
        lv = SC.levels(n, spacing)
        assert [float(v) for v in MODEL._log_snr_levels(n, spacing)] == [float(v) for v in lv]
        worst = 0.0
        for i in range(n):
            want = SC.ddpm64(lv[i], lv[i + 1])
            got = SV.step_coefficients(float(lv[i]), float(lv[i + 1]), 1.0)
            worst = max(worst, *(abs(a - b) for a, b in zip(got, want)))
        print(f"N = {n} {spacing}: max |ddim(eta = 1) - ddpm| over A, B, S = {worst:.2e}")
        assert worst <= 1e-12, worst


@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("ddim", 0.5), ("ddim", 1.0), ("dpmpp2m", 0.0)])
@pytest.mark.parametrize("spacing", ["time", "logsnr"])
def test_the_stored_scalars_are_the_float64_tables_rounded_once(sampler, eta, spacing):
    n = 6
    lv = SC.levels(n, spacing)
    plain, _ = MODEL._schedule(n) if spacing == "time" else MODEL._schedule(n, step_spacing=spacing)
    scalars, log_snrs = MODEL._schedule(n, sampler, eta, spacing)
    assert log_snrs == [float(v) for v in lv[:-1]]
    for i, (s, p) in enumerate(zip(scalars, plain)):
        a_, b_, s_ = SC.ddim64(lv[i], lv[i + 1], eta)
        for f in ("alpha", "sigma", "alpha_next", "sigma_next"):       # computed exactly as for ddpm: sigma_next feeds the ring re-noise
            assert getattr(s, f) == getattr(p, f), f
        assert s.sigma_next == float((-lv[i + 1]).sigmoid().sqrt())
        assert s.one_minus_c == float(np.float32(a_ * s.alpha / s.alpha_next)) and s.c == float(np.float32(b_ / s.alpha_next))
        assert s.noise_scale == float(np.float32(s_)) and (s.noise_scale == 0.0) == (eta == 0.0)
        # what the kernel computes with: within fp32 rounding of the float64 tables; alpha_next * c is B, the weight the guidance reads
        ga, gb, _ = _abs_table([s])[0]
        assert abs(ga - a_) <= 4 * 2.0 ** -24 * abs(a_) and abs(gb - b_) <= 4 * 2.0 ** -24 * abs(b_)
    if spacing == "logsnr":
        assert abs(log_snrs[0] + 10.0) < 1e-3 and abs(float(lv[-1]) - 9.21) < 1e-2
        gaps = np.diff([float(v) for v in lv])
        assert np.abs(gaps - gaps.mean()).max() < 1e-5


def test_the_history_weights():
    for n, spacing, first in ((6, "logsnr", 0), (6, "time", 0), (6, "time", 2), (4, "logsnr", 0), (2, "logsnr", 0), (1, "time", 0)):
        lv = SC.levels(n, spacing)
        got, want = SV.history_weights(lv, first), SC.weights64(lv, first)
        assert len(got) == n and np.allclose(got, want, rtol=0, atol=1e-15), (n, spacing, first)
        assert all(w == 0.0 for w in got[:first + 1]) and got[-1] == 0.0          # first executed step, last step
        assert all(w > 0.0 for w in got[first + 1:n - 1])
    lv = SC.levels(6, "logsnr")                          # uniform in the log-SNR: r = 1, w = B / 2
    for i, w in enumerate(SV.history_weights(lv)[1:5], start=1):
        assert abs(w - SC.ddim64(lv[i], lv[i + 1], 0.0)[1] / 2) <= 1e-6


# ------------------------------------------------------------------------------------------- (b) the solvers' order
def _gain_error(n, sampler, spacing):
    scalars, _ = MODEL._schedule(n, sampler, 0.0, spacing)
    lv = MODEL._log_snr_levels(n, spacing)
    weights = SV.history_weights(lv) if sampler == "dpmpp2m" else [0.0] * n
    return SC.gain_error([t[:2] for t in _abs_table(scalars)], weights, [float(v) for v in lv])


def test_ddim_is_first_order_and_2m_second_order_on_the_closed_form_case():
    ddim = {n: _gain_error(n, "ddim", "logsnr") for n in (16, 32, 64, 100)}
    two_m = {n: _gain_error(n, "dpmpp2m", "logsnr") for n in (16, 20, 32, 64)}
    print("logsnr spacing, relative gain error: DDIM " + ", ".join(f"N={n}: {e:.2e}" for n, e in ddim.items())
          + "; 2M " + ", ".join(f"N={n}: {e:.2e}" for n, e in two_m.items()))
    for a, b in ((16, 32), (32, 64)):
        assert 1.7 <= ddim[a] / ddim[b] <= 2.2, (a, b, ddim[a] / ddim[b])
        assert two_m[a] / two_m[b] >= 3.0, (a, b, two_m[a] / two_m[b])
    assert two_m[20] < ddim[100]
    for n in (10, 16, 20, 50, 100):                      # the reference's spacing: the last step jumps several units of log-SNR
        a, b = _gain_error(n, "dpmpp2m", "time"), _gain_error(n, "ddim", "time")
        print(f"time spacing N={n}: 2M (first-order last step) {a:.2e}, DDIM {b:.2e}")
        assert a < b, (n, a, b)


# ------------------------------------------------------------------------------------------- the restated loop
def test_the_restated_loop_as_ddpm_is_the_oracles_loop_within_fp32_rounding():
    case = G.E2E_CASES["tile256"]
    _, cond = G.e2e_input("tile256")
    want, trace = G.e2e_oracle("tile256", False)
    sd, cfg, label = O.strip_model_prefix(G.state_dict()), O.UnetCfg(dim=G.DIM), torch.tensor([G.LABEL])
    state = torch.get_rng_state()
    with torch.inference_mode():
        torch.manual_seed(case["seed"])
        got_trace = {}
        got = SC.solver_tiled_sample(sd, cfg, cond, label, batch_size=case["batch_size"], num_sample_steps=case["steps"], trace=got_trace)
        after = torch.get_rng_state()
        torch.manual_seed(case["seed"])
        O.tiled_sample(sd, cfg, cond, label, batch_size=case["batch_size"], num_sample_steps=case["steps"])
        assert torch.equal(after, torch.get_rng_state())                 # the same draws
    torch.set_rng_state(state)
    # the update is formed in float64 from the float64 table instead of fp32: a few fp32 roundings of values below 4, per step
    assert float((got - want).abs().max()) <= 1e-4
    assert max(float((a - b).abs().max()) for a, b in zip(got_trace["img"], trace["img"])) <= 1e-4
    assert O.log_snr_linear(torch.tensor(1.0)) < -9                      # the oracle's schedule is back in place


# ------------------------------------------------------------------------------------------- (c) C ABI, refusals, resources
def test_entries_are_declared_prototyped_and_exported_by_a_library_of_their_own():
    header = open(os.path.join(ROOT, "include", "srgd_solver.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(srgd_[a-z0-9_]+)\s*\(", flat))
    assert declared == ENTRIES == set(SV.PROTOTYPES)
    for name, (_, argtypes) in SV.PROTOTYPES.items():
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", flat).group(1).strip()
        assert (0 if params == "void" else len(params.split(","))) == len(argtypes), name
    fields = re.search(r"typedef struct srgd_solver_image \{(.*?)\}", flat, flags=re.S).group(1)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    assert names == [f[0] for f in SV.SolverImage._fields_] and C.sizeof(SV.SolverImage) == 32
    assert os.path.exists(SV.LIB_PATH), "build the library first (python -m srgd_amd.build)"
    assert _exports(SV.LIB_PATH) == ENTRIES
    assert SV.lib().srgd_solver_last_error() is not None                       # binds every prototype
    for mod in (_lib, MX, EN, CS, BP, GD):               # the six other libraries keep their export tables
        assert _exports(mod.LIB_PATH) == set(mod.PROTOTYPES), mod.__name__
        assert not any("solver" in n for n in _exports(mod.LIB_PATH)), mod.__name__
        assert not set(SV.PROTOTYPES) & set(mod.PROTOTYPES)
    for phrase in ("d = x_start - x_prev;  if (w != 0) img = img + w * d;  x_prev = x_start",
                   "With w == 0 img is neither read nor written", "Everything outside the boxes keeps its bytes in all three buffers",
                   "There are no clamps", "bit-identical to the call on that image alone",
                   "Asynchronous on `stream`; no allocation, no synchronisation"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", header), phrase


def test_refusals_need_no_gpu():
    # every refusal is decided on the host before anything is launched, so it can be checked here: -1 and a message
    lib = SV.lib()
    at = lambda v: C.c_void_p(v)                           # noqa: E731
    img, xs, xp = 1 << 24, 2 << 24, 3 << 24                # never dereferenced: a refused call launches nothing

    def rec(**kw):
        base = dict(canvas_off=0, Hp=256, Wp=256, top=3, left=5, h=20, w=31)
        return SV.SolverImage(**dict(base, **kw))

    def call(images=None, n=None, **kw):
        images = [rec()] if images is None else images
        a = dict(dict(img=at(img), xs=at(xs), xp=at(xp), w=0.5), **kw)
        arr = (SV.SolverImage * len(images))(*images) if images != "null" else None
        rc = lib.srgd_solver_history_step(a["img"], a["xs"], a["xp"], arr, len(images) if n is None else n, a["w"], None)
        return rc, lib.srgd_solver_last_error().decode()
    canvas = 4 * 3 * 256 * 256
    cases = {"null": [dict(img=None), dict(xs=None), dict(xp=None), dict(images="null", n=1)],
             "n must be": [dict(n=0), dict(n=-1)],
             "bad size": [dict(images=[rec(h=0)]), dict(images=[rec(w=0)]), dict(images=[rec(h=-2)]),
                          dict(images=[rec(), rec(canvas_off=3 * 65536, w=-1)])],
             "bad canvas": [dict(images=[rec(Hp=0)]), dict(images=[rec(Wp=-1)]), dict(images=[rec(Hp=26755, Wp=26755, top=0, left=0)])],
             "leaves its canvas": [dict(images=[rec(top=-1)]), dict(images=[rec(left=-1)]), dict(images=[rec(top=237)]),
                                   dict(images=[rec(left=226)]), dict(images=[rec(h=254)]), dict(images=[rec(Wp=35)]),
                                   dict(images=[rec(top=2 ** 31 - 1)])],
             "offset outside": [dict(images=[rec(canvas_off=-1)]), dict(images=[rec(canvas_off=1 << 40)])],
             "finite": [dict(w=float("nan")), dict(w=float("inf")), dict(w=float("-inf"))],
             "4-byte aligned": [dict(img=at(img + 2)), dict(xs=at(xs + 1)), dict(xp=at(xp + 3))],
             "overlapping canvases": [dict(images=[rec(), rec()]), dict(images=[rec(), rec(canvas_off=3 * 65536 - 1)]),
                                      dict(images=[rec(canvas_off=3 * 65536), rec(), rec(canvas_off=6 * 65536 - 7)])],
             "overlapping buffers": [dict(xs=at(img)), dict(xs=at(img + canvas - 4)), dict(xs=at(img - canvas + 4)), dict(xp=at(img + 4)),
                                     dict(xp=at(xs + canvas - 4)), dict(xp=at(xs))]}
    for word, variants in cases.items():
        for kw in variants:
            rc, msg = call(**kw)
            assert rc == -1 and word in msg and msg.startswith("srgd_solver_history_step: "), (kw, msg)
    assert 3 * 26755 * 26755 >= 2 ** 31 > 3 * 26754 * 26754


def test_host_side_checks_of_the_module():
    assert SV.SAMPLERS == ("ddpm", "ddim", "dpmpp2m") and SV.SPACINGS == ("time", "logsnr")
    assert SV.check_sampler() == ("ddpm", None, "time") and SV.is_default(*SV.check_sampler())
    assert SV.check_sampler("ddim") == ("ddim", 0.0, "time") and SV.check_sampler("ddim", 1, "logsnr") == ("ddim", 1.0, "logsnr")
    assert SV.check_sampler("dpmpp2m") == ("dpmpp2m", 0.0, "time") and SV.check_sampler("dpmpp2m", 0.0) == ("dpmpp2m", 0.0, "time")
    assert not SV.is_default("ddim", 0.0, "time") and not SV.is_default("ddpm", None, "logsnr")
    for bad in (dict(sampler="euler"), dict(sampler=None), dict(step_spacing="karras"), dict(step_spacing=None), dict(eta=0.0),
                dict(eta=1.0), dict(sampler="ddim", eta=-0.1), dict(sampler="ddim", eta=1.5), dict(sampler="ddim", eta=float("nan")),
                dict(sampler="ddim", eta="0"), dict(sampler="ddim", eta=True), dict(sampler="dpmpp2m", eta=0.5),
                dict(sampler="dpmpp2m", eta=1)):
        with pytest.raises(ValueError, match="sampler|eta|step_spacing"):
            SV.check_sampler(**bad)
    recs = SV.records([(0, 37, 53, 3, 5, 20, 31), (3 * 37 * 53 + 1, 8, 8, 1, 1, 6, 6)])
    assert len(recs) == 2 and (recs[1].canvas_off, recs[1].Hp, recs[1].Wp, recs[1].top, recs[1].left, recs[1].h, recs[1].w) == \
        (5884, 8, 8, 1, 1, 6, 6)
    for bad in ([], [(0, 37, 53, 3, 5, 35, 31)], [(0, 37, 53, 3, 5, 20, 49)], [(0, 37, 53, -1, 5, 20, 31)], [(-1, 37, 53, 3, 5, 20, 31)],
                [(0, 37, 53, 3, 5, 0, 31)], [(0, 26755, 26755, 0, 0, 20, 20)]):
        with pytest.raises(ValueError, match="solver"):
            SV.records(bad)
    f32 = lambda n: torch.zeros(n, dtype=torch.float32)                       # noqa: E731
    recs = SV.records([(0, 37, 53, 3, 5, 20, 31)])
    ok = dict(img=f32(3 * 37 * 53), x_start=f32(3 * 37 * 53), x_prev=f32(3 * 37 * 53), recs=recs, w=0.5)
    for kw in (dict(w=float("nan")), dict(w=float("inf")), dict(w="1"), dict(w=True), dict(recs=[recs[0]]), dict(recs=None),
               dict(img=f32(3 * 37 * 53).double()), dict(x_start=f32(3 * 37 * 53 - 1)), dict(x_prev=f32(10)), dict(x_prev=None)):
        with pytest.raises(ValueError, match="solver"):
            SV.history_step_flat(**dict(ok, **kw))
    with pytest.raises(_lib.SrgdHipError, match="no CPU fallback"):          # a missing GPU is an error, never another path
        SV.history_step_flat(**ok)
    assert list(inspect.signature(SV.history_step_flat).parameters) == ["img", "x_start", "x_prev", "recs", "w"]
    source = inspect.getsource(SV)
    assert "torch.empty" not in source and "torch.zeros" not in source and ".clone(" not in source      # the caller owns every buffer


def test_the_numpy_statement_of_the_kernel():
    recs = SC.KERNEL_GROUPS["solo"]
    img, xs, xp = SC.kernel_buffers(recs, 1)
    img0, xp0 = img.copy(), xp.copy()
    SC.history_np(img, xs, xp, recs, 0.37)
    box = (slice(None), slice(3, 23), slice(5, 36))
    v = lambda a: a.reshape(3, 37, 53)                                        # noqa: E731
    outside = np.ones((3, 37, 53), dtype=bool)
    outside[box] = False
    assert np.array_equal(v(img)[outside], v(img0)[outside]) and np.array_equal(v(xp)[outside], v(xp0)[outside])
    assert np.array_equal(v(xp)[box], v(xs)[box])
    want = v(img0)[box].astype(np.float64) + 0.37 * (v(xs)[box].astype(np.float64) - v(xp0)[box])
    assert np.abs(v(img)[box] - want).max() <= 3 * 2.0 ** -24 * 4
    img2, _, xp2 = img0.copy(), None, xp0.copy()
    xp2[5] = np.nan
    SC.history_np(img2, xs, xp2, recs, 0.0)
    assert np.array_equal(img2, img0)


def test_the_kernel_does_not_spill_and_uses_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_resources import kernel_table
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "solver.hip")) if "solver_" in r["name"]]
    assert [r["name"] for r in rows] == ["solver_history_kernel"]
    for r in rows:
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0, r
        assert r["vgpr"] <= 64, r                          # eight waves per SIMD: the kernel only moves memory


# ------------------------------------------------------------------------------------------- flags and keywords
def test_the_flags_parse():
    args = INF.parse_args(_argv())
    assert (args.sampler, args.eta, args.step_spacing) == ("ddpm", None, "time")
    args = INF.parse_args(_argv("--sampler", "ddim", "--eta", "0.5", "--step_spacing", "logsnr"))
    assert (args.sampler, args.eta, args.step_spacing) == ("ddim", 0.5, "logsnr")
    args = INF.parse_args(_argv("--sampler", "dpmpp2m", "--step_spacing", "logsnr", "--consistency_guidance", "1", "--samples", "3"))
    assert (args.sampler, args.eta, args.step_spacing, args.consistency_guidance) == ("dpmpp2m", None, "logsnr", 1.0)
    assert INF.parse_args(_argv("--sampler", "dpmpp2m", "--eta", "0")).eta == 0.0
    for bad in (("--eta", "0.5"), ("--sampler", "ddpm", "--eta", "0"), ("--sampler", "ddim", "--eta", "1.5"),
                ("--sampler", "ddim", "--eta", "-0.1"), ("--sampler", "ddim", "--eta", "nan"), ("--sampler", "dpmpp2m", "--eta", "0.5")):
        with pytest.raises(SystemExit, match="--eta"):
            INF.parse_args(_argv(*bad))
    for bad in (("--sampler", "euler"), ("--step_spacing", "karras"), ("--eta", "some")):
        with pytest.raises(SystemExit):
            INF.parse_args(_argv(*bad))


def test_every_keyword_defaults_to_today_and_the_untiled_sample_has_none():
    ddpm, edm = MODEL.ConditionalContinuousTimeGaussianDiffusionSR, MODEL.ConditionalElucidatedDiffusionSR
    for fn in (INF.sr_target_image, INF.sr_target_images, INF.sr_target_images_mixed, INF.sr_target_images_seeded,
               INF.batch_sr_target_images, ddpm.tiled_sample, edm.tiled_sample):
        params = inspect.signature(fn).parameters
        assert (params["sampler"].default, params["eta"].default, params["step_spacing"].default) == ("ddpm", None, "time"), fn.__qualname__
    for fn in (ddpm.sample, edm.sample, edm.sample_org, edm.sample_using_dpmpp):
        assert not set(KEYWORDS) & set(inspect.signature(fn).parameters), fn.__qualname__
    assert INF._sampler_kw() == {} and INF._sampler_kw("ddpm", None, "time") == {} and INF._sampler_kw(None, None, None) == {}
    assert INF._sampler_kw("ddim") == {"sampler": "ddim"} and INF._sampler_kw("ddim", 0.0) == {"sampler": "ddim", "eta": 0.0}
    assert INF._sampler_kw(step_spacing="logsnr") == {"step_spacing": "logsnr"}
    assert INF._sampler_kw("dpmpp2m", None, "logsnr") == {"sampler": "dpmpp2m", "step_spacing": "logsnr"}


class _Unused:
    """A sampler whose every attribute access fails the test: ``tiled_sample`` must refuse before it touches the model."""
    canvas_group = None

    def __getattr__(self, name):
        raise AssertionError(f"the sampler was touched ({name}) before the arguments were checked")


class _Sharded(_Unused):
    canvas_group = object()


def test_the_ddpm_wrapper_checks_the_keywords_on_entry():
    fn = inspect.unwrap(MODEL.ConditionalContinuousTimeGaussianDiffusionSR.tiled_sample)
    cond = torch.zeros(1, 3, 256, 256)
    for bad in (dict(sampler="euler"), dict(step_spacing="karras"), dict(eta=0.0), dict(sampler="ddpm", eta=1.0),
                dict(sampler="ddim", eta=1.5), dict(sampler="ddim", eta=-1), dict(sampler="ddim", eta="0.5"),
                dict(sampler="dpmpp2m", eta=0.25)):
        with pytest.raises(ValueError, match="sampler|eta|step_spacing"):
            fn(_Unused(), condition_x=cond, **bad)
        with pytest.raises(ValueError, match="sampler|eta|step_spacing"):
            fn(_Unused(), condition_x=[cond, cond], seeds=[1, 2], **bad)


def test_a_sharded_canvas_refuses_dpmpp2m_and_the_edm_wrapper_every_non_default_value():
    fn = inspect.unwrap(MODEL.ConditionalContinuousTimeGaussianDiffusionSR.tiled_sample)
    cond = torch.zeros(1, 3, 256, 256)
    with pytest.raises(NotImplementedError, match="dpmpp2m.*canvas_group"):
        fn(_Sharded(), condition_x=cond, sampler="dpmpp2m")
    with pytest.raises(NotImplementedError, match="dpmpp2m.*canvas_group"):
        fn(_Sharded(), condition_x=cond, sampler="dpmpp2m", eta=0, step_spacing="logsnr")
    # ddim and step_spacing only change tables: a sharded canvas takes them (the call gets past the refusals to the sampler itself)
    for kw in (dict(sampler="ddim", eta=0.5), dict(step_spacing="logsnr")):
        with pytest.raises(AssertionError, match="the sampler was touched"):
            fn(_Sharded(), condition_x=cond, **kw)
    # the existing refusals stay in front of it
    with pytest.raises(NotImplementedError, match="consistency_guidance on a canvas sharded"):
        fn(_Sharded(), condition_x=cond, sampler="ddim", consistency_guidance=0.5)
    edm = inspect.unwrap(MODEL.ConditionalElucidatedDiffusionSR.tiled_sample)
    for kw in (dict(sampler="ddim"), dict(sampler="dpmpp2m"), dict(step_spacing="logsnr"), dict(sampler="ddim", eta=0.0)):
        with pytest.raises(NotImplementedError, match="DDPM sampler only"):
            edm(_Unused(), condition_x=cond, **kw)
    with pytest.raises(ValueError, match="sampler"):
        edm(_Unused(), condition_x=cond, sampler="heun")
    with pytest.raises(ValueError, match="eta"):
        edm(_Unused(), condition_x=cond, eta=0.0)


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


def test_the_batch_loop_hands_the_keywords_on_only_when_they_are_not_the_default(tmp_path, monkeypatch):
    calls = []
    _fake_samplers(monkeypatch, calls)
    indir = _inputs(tmp_path, {"a": (64, 64), "b": (64, 64), "c": (48, 64)})
    run = lambda tag, **kw: INF.batch_sr_target_images(str(indir), str(tmp_path / tag), None, seed=71, **kw)  # noqa: E731
    for tag, kw in (("solo", {}), ("same", dict(lockstep=2)), ("mixed", dict(lockstep_tiles=8)), ("seeded", dict(samples=2))):
        calls.clear()
        run(tag + "_off", **kw)
        run(tag + "_default", sampler="ddpm", eta=None, step_spacing="time", **kw)
        assert calls and all(not set(KEYWORDS) & set(c[2]) for c in calls), tag
        kinds_off = [c[:2] for c in calls[:len(calls) // 2]]
        calls.clear()
        run(tag + "_2m", sampler="dpmpp2m", step_spacing="logsnr", **kw)
        assert [c[:2] for c in calls] == kinds_off, tag
        assert all(c[2]["sampler"] == "dpmpp2m" and c[2]["step_spacing"] == "logsnr" and "eta" not in c[2] for c in calls), tag
        calls.clear()
        run(tag + "_ddim", sampler="ddim", eta=0.5, **kw)
        assert all(c[2]["sampler"] == "ddim" and c[2]["eta"] == 0.5 and "step_spacing" not in c[2] for c in calls), tag
        assert sorted(os.listdir(tmp_path / (tag + "_2m"))) == sorted(os.listdir(tmp_path / (tag + "_off")))
    calls.clear()
    with pytest.raises(ValueError, match="eta"):
        run("bad", sampler="dpmpp2m", eta=0.5)
    assert not calls                                            # before anything is sampled


def test_the_sr_functions_hand_the_keywords_to_tiled_sample_only_when_they_are_not_the_default(monkeypatch):
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
        run(sampler="ddpm", eta=None, step_spacing="time")
        assert len(seen) == 2 and all(not set(KEYWORDS) & set(kw) for kw in seen)
        run(sampler="ddim", eta=0.0, step_spacing="logsnr")
        assert (seen[2]["sampler"], seen[2]["eta"], seen[2]["step_spacing"]) == ("ddim", 0.0, "logsnr")
        assert set(seen[2]) - set(seen[0]) == set(KEYWORDS)
        run(sampler="dpmpp2m")
        assert set(seen[3]) - set(seen[0]) == {"sampler"}
