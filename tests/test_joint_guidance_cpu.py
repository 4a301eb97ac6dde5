"""Joint guidance (``tiled_sample(joint_guidance=True)``, srgd_sampler_step with passes = 3) - what needs no GPU: the yardsticks of
tests/joint_guidance_cases.py against the oracle, the step table, the refusals, the flag, the header, the binding and the resource table,
and the sensitivity of the one-step check the GPU suite makes."""
import inspect
import os
import re
import subprocess

import pytest
import torch

from oracle import srgd_oracle as O
from srgd_amd import _lib
from srgd_amd import inference as INF
from srgd_amd import model as MODEL
from tests import joint_guidance_cases as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = "Currently, you cannot specify both cond_scale and class_cond_scale at the same time."


# ------------------------------------------------------------------------------------------------ (a)
def test_the_combine_reduces_to_either_single_guidance():
    g = torch.Generator().manual_seed(7)
    e, n_c, n_l = (torch.randn(2, 3, 16, 16, generator=g, dtype=torch.float64) for _ in range(3))
    for s in (0.0, 0.5, 1.5, 2.0, 7.25):
        # a handful of float64 roundings on values of magnitude <= 8 |s|
        tol = 16 * 2.0 ** -52 * (1 + abs(s)) * 8
        assert (J.combine64(e, n_c, n_l, s, 1.0) - J.cond_guided64(e, n_c, s)).abs().max() <= tol          # model.py:3150
        assert (J.combine64(e, n_c, n_l, 1.0, s) - J.class_guided64(e, n_l, s)).abs().max() <= tol         # model.py:3154
    assert torch.equal(J.combine64(e, n_c, n_l, 1.0, 1.0), e)
    # upstream's commented-out four-pass form does not reduce: with s_l = 1 it still reads the fully unconditional prediction
    assert not torch.equal(J.combine64(e, n_c, n_l, 1.5, 3.0), J.combine64(e, n_c, n_l, 3.0, 1.5))
    nan = e.clone()
    nan[0, 0, 0, 0] = float("nan")
    for args in ((nan, n_c, n_l), (e, nan, n_l), (e, n_c, nan)):     # nothing selects a non-finite prediction away
        out = J.combine64(*args, 1.5, 2.0)
        assert torch.isnan(out[0, 0, 0, 0]) and torch.isfinite(out).sum() == out.numel() - 1


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("kw", [dict(cond_scale=1.5, guidance_start_steps=1), dict(class_cond_scale=2.0)], ids=["cond", "class"])
def test_the_restated_loop_is_the_oracle_when_one_scale_is_one(kw):
    sd, cfg = O.strip_model_prefix(J.state_dict()), O.UnetCfg(dim=J.DIM)
    cond = J.condition(256, 256)
    run = lambda fn: J.with_seed(5, lambda: fn(sd, cfg, cond, J.label(), num_sample_steps=2, **kw))
    assert torch.equal(run(J.joint_tiled_sample), run(O.tiled_sample))


# ------------------------------------------------------------------------------------------------ the step table
def test_step_guidance_table_for_staggered_starts():
    f = MODEL._step_guidance
    # condition guidance from step 2, class guidance from step 1
    want = [(1, 0, 1.0), (2, 1, 2.0), (3, 3, (1.5, 2.0)), (3, 3, (1.5, 2.0))]
    assert [f(i, 1.5, 2, 2.0, 1, True) for i in range(4)] == want
    # the other way round: condition guidance alone first
    assert [f(i, 1.5, 1, 2.0, 3, True) for i in range(4)] == [(1, 0, 1.0), (2, 2, 1.5), (2, 2, 1.5), (3, 3, (1.5, 2.0))]
    # without the keyword: today's table, positionally and by default
    old = [(1, 0, 1.0), (2, 1, 2.0), (2, 2, 1.5), (2, 2, 1.5)]
    assert [f(i, 1.5, 2, 2.0, 1) for i in range(4)] == old == [f(i, 1.5, 2, 2.0, 1, False) for i in range(4)]
    # one scale at 1: the keyword changes nothing
    for i in range(4):
        assert f(i, 1.5, 2, 1.0, 0, True) == f(i, 1.5, 2, 1.0, 0) and f(i, 1.0, 0, 2.0, 1, True) == f(i, 1.0, 0, 2.0, 1)
    # a joint launch holds at most the entries of a two-pass launch
    for sb in range(1, 130):
        t = MODEL._launch_tiles(3, sb)
        assert t >= 1 and (3 * t <= 2 * sb or sb == 1) and t == max(1, 2 * sb // 3)
        assert MODEL._launch_tiles(2, sb) == MODEL._launch_tiles(1, sb) == sb


# ------------------------------------------------------------------------------------------------ refusals
class _Unused:
    """A sampler whose every attribute access fails the test: the refusals come before the model is touched."""
    canvas_group = None

    def __getattr__(self, name):
        raise AssertionError(f"the sampler was touched ({name}) before the arguments were checked")


class _Sharded(_Unused):
    canvas_group = object()


def test_refusals():
    fn = inspect.unwrap(MODEL.ConditionalContinuousTimeGaussianDiffusionSR.tiled_sample)
    cond = torch.zeros(1, 3, 256, 256)
    lab = torch.tensor([0])
    forms = (dict(condition_x=cond), dict(condition_x=[cond, cond]), dict(condition_x=[cond, cond], seeds=[1, 2]),
             dict(condition_x=torch.zeros(2, 3, 256, 256), seeds=[1, 2]))
    forms = tuple(dict(f, num_sample_steps=4) for f in forms)
    for form in forms:
        with pytest.raises(NotImplementedError) as err:                # without the keyword: as upstream, the same text
            fn(_Unused(), class_label=lab, cond_scale=2.0, class_cond_scale=2.0, **form)
        assert str(err.value) == BOTH
        with pytest.raises(NotImplementedError) as err:
            fn(_Unused(), class_label=lab, cond_scale=2.0, class_cond_scale=2.0, joint_guidance=False, **form)
        assert str(err.value) == BOTH
        with pytest.raises(ValueError, match="class_label"):
            fn(_Unused(), class_label=None, cond_scale=2.0, class_cond_scale=2.0, joint_guidance=True, **form)
        with pytest.raises(ValueError, match="finite"):
            fn(_Unused(), class_label=lab, cond_scale=float("inf"), class_cond_scale=2.0, joint_guidance=True, **form)
        with pytest.raises(NotImplementedError, match="canvas_group"):
            fn(_Sharded(), class_label=lab, cond_scale=2.0, class_cond_scale=2.0, joint_guidance=True, **form)
    edm = inspect.unwrap(MODEL.ConditionalElucidatedDiffusionSR.tiled_sample)
    untiled = inspect.unwrap(MODEL.ConditionalContinuousTimeGaussianDiffusionSR.sample)

    class _Steps(_Unused):
        num_sample_steps = 4
    for jg in (False, True):
        with pytest.raises(NotImplementedError) as err:
            edm(_Steps(), condition_x=cond, class_label=lab, cond_scale=2.0, class_cond_scale=2.0, joint_guidance=jg)
        assert str(err.value) == BOTH
        with pytest.raises(NotImplementedError) as err:
            untiled(_Steps(), condition_x=cond, class_label=lab, cond_scale=2.0, class_cond_scale=2.0, joint_guidance=jg)
        assert str(err.value) == BOTH


# ------------------------------------------------------------------------------------------------ the flag
def _argv(*extra):
    return ["-c", "x", "-m", "w", "--input_dir", "i", "--output_dir", "o", *extra]


def test_the_flag_parses_and_is_handed_on_only_when_set():
    assert INF.parse_args(_argv()).joint_guidance is False
    a = INF.parse_args(_argv("--joint_guidance", "--cond_scale", "1.5", "--class_cond_scale", "2.0"))
    assert a.joint_guidance is True and a.cond_scale == 1.5 and a.class_cond_scale == 2.0
    assert INF._joint_kw(False) == {} and INF._joint_kw(True) == {"joint_guidance": True}
    ddpm, edm = MODEL.ConditionalContinuousTimeGaussianDiffusionSR, MODEL.ConditionalElucidatedDiffusionSR
    for fn in (INF.sr_target_image, INF.sr_target_images, INF.sr_target_images_mixed, INF.sr_target_images_seeded,
               INF.batch_sr_target_images, ddpm.tiled_sample, edm.tiled_sample, ddpm.sample):
        assert inspect.signature(fn).parameters["joint_guidance"].default is False, fn.__qualname__
    src = inspect.getsource(INF.main)
    assert "_joint_kw(args.joint_guidance)" in src


# ------------------------------------------------------------------------------------------------ the build
def test_the_joint_form_rides_the_existing_entries():
    # the export table stays as it is: the joint step is srgd_sampler_step / _step_tiles with passes = 3, the class scale in guidance_kind
    header = open(os.path.join(ROOT, "include", "srgd_hip.h")).read()
    assert "e + (s_c - 1) (e - n_c) + (s_l - 1) (e - n_l)" in header and "fma(wl, dl, r)" in header and "passes = 3" in header
    assert not any("joint" in name for name in _lib.PROTOTYPES)
    assert len(_lib.PROTOTYPES["srgd_sampler_step"][1]) == 13 and len(_lib.PROTOTYPES["srgd_sampler_step_tiles"][1]) == 16
    assert os.path.exists(_lib.LIB_PATH), "build the library first (python -m srgd_amd.build)"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert {n for n in exported if n.startswith("srgd_")} == set(_lib.PROTOTYPES)
    from srgd_amd.engine import HipEngine
    import struct
    for v in (2.0, 3.0, 0.0, -1.5, 1.0000001, float("inf")):
        k = HipEngine._joint_kind(v)
        assert -2 ** 31 <= k < 2 ** 31 and struct.unpack("<f", struct.pack("<i", k))[0] == struct.unpack("<f", struct.pack("<f", v))[0]
    calls = []

    class Probe:
        _joint_kind = staticmethod(HipEngine._joint_kind)

        def sampler_step(self, *a):
            calls.append(("step",) + a)

        def sampler_step_tiles(self, *a):
            calls.append(("tiles",) + a)
    HipEngine.sampler_step_joint(Probe(), 4, "img", "cc", "xs", "nt", "nc", 1.5, 2.0, 6, 9)
    HipEngine.sampler_step_joint_tiles(Probe(), 4, 1, 2, True, "img", "cc", "xs", "nt", "nc", 1.5, 2.0, 6, 9)
    two = HipEngine._joint_kind(2.0)
    assert calls == [("step", 4, "img", "cc", "xs", "nt", "nc", 3, two, 1.5, 6, 9),
                     ("tiles", 4, 1, 2, True, "img", "cc", "xs", "nt", "nc", 3, two, 1.5, 6, 9)]


def test_the_final_step_kernels_do_not_spill():
    from tools.kernel_resources import kernel_table
    # two-pass and three-pass instances, bf16 and fp32 each (c++filt does not demangle the bf16 names: counted, not parsed)
    rows = [r for r in kernel_table(os.path.join(ROOT, "srgd_amd", "csrc", "sampler.hip"))
            if "final_step_kernel" in r["name"] and "edm" not in r["name"]]
    assert len(rows) == 4, [r["name"] for r in rows]
    assert sum("final_step_kernel<float, true>" in r["name"] for r in rows) == 1, [r["name"] for r in rows]
    for r in rows:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["lds"] == 3 * 256 * 4, r                               # eps[3][256]
        assert 0 < r["vgpr"] <= 128, r                                  # 256 threads: at least four waves per SIMD


# ------------------------------------------------------------------------------------------------ sensitivity
def test_every_mutant_moves_x_start_far_beyond_the_one_step_bar():
    # the one-step GPU check (test_joint_guidance_gpu.py, test 2) on its own first tile: dim 16, WEIGHT_SEED, s_c = 1.5, s_l = 3.0.
    # Each mutant of (b)'s joint step must move x_start by more than 100 x the cap that test puts on its own bar.
    sd, cfg = O.strip_model_prefix(J.state_dict(J.WEIGHT_SEED)), O.UnetCfg(dim=J.DIM)
    x, c01, z = J.one_step_inputs(256, 256)
    cond = c01 * 2 - 1
    ts = torch.linspace(1.0, 0.0, J.ONE_STEP_STEPS + 1)
    t, t_next = ts[J.ONE_STEP_INDEX], ts[J.ONE_STEP_INDEX + 1]
    memo = {}

    def unet(sd_, cfg_, x_, ls, lab, cnd):
        key = (lab is None, cnd is None)
        if key not in memo:
            memo[key] = O.unet_forward(sd_, cfg_, x_, ls, lab, cnd)
        return memo[key]
    with torch.inference_mode():
        step = lambda m: J.joint_predict_and_step(sd, cfg, x, t, t_next, cond, J.label(), J.SENS_S_C, J.SENS_S_L, O.ReplayNoise([z]),
                                                  mutant=m, unet=unet)
        _, x0 = step(None)
        assert float((x0.abs() < 1).float().mean()) > 0.25             # enough of the prediction is off the clamp
        moved = {m: float((step(m)[1].double() - x0.double()).abs().max()) for m in J.MUTANTS}
    print("x_start moved by", moved, "needed", J.MUTANT_FACTOR * J.ONE_STEP_BAR_CAP)
    assert len(memo) == 3
    for m, d in moved.items():
        assert d > J.MUTANT_FACTOR * J.ONE_STEP_BAR_CAP, (m, d)
