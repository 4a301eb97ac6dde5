"""Precision schedules without a GPU: the parser and the planner against a table, every refusal of the module, of ``tiled_sample``
(before the model is touched) and of the command line, and what the command line hands on with and without the flag."""
import inspect
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from srgd_amd import inference as INF
from srgd_amd import model as MODEL
from srgd_amd import precision_schedule as PS


# ------------------------------------------------------------------------------------------------ parser and planner
PLANS = [
    ("bf16:3,f16x3", 5, ["bf16"] * 3 + ["f16x3"] * 2),
    ("bf16,f16x3:2", 5, ["bf16"] * 3 + ["f16x3"] * 2),
    ("fp32:5", 5, ["fp32"] * 5),                                        # fully counted
    ("bf16:5,f16x3", 5, ["bf16"] * 5),                                  # the rest entry gets nothing
    ("bf16:2,bf16:1,f16x3", 5, ["bf16"] * 3 + ["f16x3"] * 2),           # adjacent entries of one name
    ("f16x3", 4, ["f16x3"] * 4),
    ("bf16:1,f16x1,f16x3:2,fp32:1", 7, ["bf16"] + ["f16x1"] * 3 + ["f16x3"] * 2 + ["fp32"]),
    (" bf16 : 3 , f16x3 ", 5, ["bf16"] * 3 + ["f16x3"] * 2),
    ("bf16:+3,f16x3", 5, ["bf16"] * 3 + ["f16x3"] * 2),
]


@pytest.mark.parametrize("spec,n,want", PLANS, ids=[p[0].strip() for p in PLANS])
def test_the_plan_of_a_schedule(spec, n, want):
    assert PS.plan_steps(spec, n) == want
    pairs = PS.parse_schedule(spec)
    assert PS.parse_schedule(pairs) == pairs and PS.parse_schedule(list(map(list, pairs))) == pairs
    assert PS.plan_steps(pairs, n) == want                              # the sequence-of-pairs spelling
    assert PS.parse_schedule(PS.format_runs(pairs)) == pairs


def test_the_parsed_entries_and_the_merged_runs():
    assert PS.parse_schedule("bf16:40,f16x3") == (("bf16", 40), ("f16x3", None))
    assert PS.parse_schedule("bf16,f16x3:10") == (("bf16", None), ("f16x3", 10))
    assert PS.parse_schedule([("bf16", 2), ("bf16", 1), ("f16x3", None)]) == PS.parse_schedule("bf16:2,bf16:1,f16x3")
    plan = PS.plan_steps("bf16:2,bf16:1,f16x3", 5)
    assert PS.plan_runs(plan) == [("bf16", 3), ("f16x3", 2)]
    assert PS.describe_plan(PS.plan_steps("bf16:40,f16x3", 50)) == "bf16 x40, f16x3 x10"
    assert PS.describe_plan(PS.plan_steps("bf16:5,f16x3", 5)) == "bf16 x5"
    assert PS.plan_runs([]) == []


def test_the_names_are_the_engines_precisions():
    from srgd_amd import engine
    assert sorted(PS.PRECISION_NAMES) == sorted(engine._PRECISIONS) and len(set(PS.PRECISION_NAMES)) == len(PS.PRECISION_NAMES)


def test_the_executed_names():
    plan = PS.plan_steps("bf16:3,f16x3:1,bf16", 6)
    assert PS.executed_names(plan) == ["bf16", "f16x3"]
    assert PS.executed_names(plan, 3) == ["f16x3", "bf16"]
    assert PS.executed_names(plan, 4) == ["bf16"]
    assert PS.executed_names(PS.plan_steps("bf16:5,f16x3", 5)) == ["bf16"]     # the rest entry's engine is never built
    assert PS.executed_names(PS.plan_steps("bf16:3,f16x3", 5), 5) == ["f16x3"]  # nothing executed: the start and end calls' engine


def test_the_module_needs_neither_torch_nor_a_gpu():
    code = ("import sys; import srgd_amd.precision_schedule as p; assert p.plan_steps('bf16:1,f16x3', 3) == ['bf16', 'f16x3', 'f16x3']; "
            "assert 'torch' not in sys.modules and 'numpy' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=MODEL.__file__.rsplit("/srgd_amd/", 1)[0])


# ------------------------------------------------------------------------------------------------ refusals of the module
BAD_SPECS = [
    ("bf17", "bf17"), ("bf16:3,half", "half"), ("BF16", "BF16"),                      # unknown names
    ("bf16:0,f16x3", "bf16:0"), ("bf16:-2,f16x3", "bf16:-2"),                         # counts of 0 or below
    ("bf16:2.5,f16x3", "bf16:2.5"), ("bf16:x", "bf16:x"), ("bf16:", "bf16:"), ("bf16:1:2", "bf16:1:2"), ("bf16:1e1", "bf16:1e1"),
    ("", "''"), ("bf16,,f16x3", "''"), ("bf16:3,", "''"), (" ", "' '"), (":3", ":3"),  # empty entries
    ("bf16,f16x3", "f16x3"), ("bf16:1,f16x3,fp32", "fp32"),                           # more than one rest entry
    ("bf16:1,f16x3:1,fp32:1,f16x1:1,bf16:1", "bf16:1"),                               # more than 4 entries
]


@pytest.mark.parametrize("spec,token", BAD_SPECS, ids=[repr(b[0]) for b in BAD_SPECS])
def test_a_malformed_schedule_is_refused_with_its_token(spec, token):
    with pytest.raises(ValueError) as err:
        PS.parse_schedule(spec)
    assert token in str(err.value) and "precision schedule" in str(err.value)
    with pytest.raises(ValueError):
        PS.plan_steps(spec, 50)


def test_malformed_pairs_are_refused():
    for bad, token in (([("bf17", 1)], "bf17"), ([("bf16", 0), ("f16x3", None)], "0"), ([("bf16", 2.0), ("f16x3", None)], "2.0"),
                       ([("bf16", True), ("f16x3", None)], "True"), ([("bf16", "2")], "'2'"), ([("", 1)], "''"), ([], "empty"),
                       ([("bf16", None), ("f16x3", None)], "f16x3"), ([("bf16", 1)] * 5, "bf16"), (["bf16"], "bf16"), ([("bf16",)], "bf16"),
                       (7, "7"), (None, "None")):
        with pytest.raises(ValueError) as err:
            PS.parse_schedule(bad)
        assert token in str(err.value), bad


def test_counts_that_do_not_fit_the_run_are_refused():
    with pytest.raises(ValueError, match="above the run's 5 steps"):
        PS.plan_steps("bf16:6,f16x3", 5)
    with pytest.raises(ValueError, match="above the run's 5 steps"):
        PS.plan_steps("bf16:3,f16x3:3", 5)
    with pytest.raises(ValueError, match="sum to 4, the run has 5 steps"):
        PS.plan_steps("bf16:3,f16x3:1", 5)
    with pytest.raises(ValueError, match="sum to 6"):
        PS.plan_steps("fp32:6", 5)
    for n in (0, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="num_sample_steps"):
            PS.plan_steps("bf16", n)


# ------------------------------------------------------------------------------------------------ refusals of tiled_sample
class _Unused:
    """A sampler whose every attribute access fails the test: the refusals come before the model is touched."""
    canvas_group = None

    def __getattr__(self, name):
        raise AssertionError(f"the sampler was touched ({name}) before the arguments were checked")


class _Sharded(_Unused):
    canvas_group = object()


def test_refusals_of_tiled_sample():
    fn = inspect.unwrap(MODEL.ConditionalContinuousTimeGaussianDiffusionSR.tiled_sample)
    cond = torch.zeros(1, 3, 300, 260)
    forms = (dict(condition_x=cond, num_sample_steps=5), dict(condition_x=[cond, cond], num_sample_steps=5),
             dict(condition_x=[cond, cond], seeds=[1, 2], num_sample_steps=5))
    for form in forms:
        for spec, token in BAD_SPECS:
            with pytest.raises(ValueError) as err:
                fn(_Unused(), precision_schedule=spec, **form)
            assert token in str(err.value), (spec, form)
        for spec in ("bf16:6,f16x3", "bf16:3,f16x3:1", "fp32:50"):                     # against the run's 5 steps
            with pytest.raises(ValueError, match="precision schedule"):
                fn(_Unused(), precision_schedule=spec, **form)
        with pytest.raises(ValueError, match="precision and precision_schedule"):
            fn(_Unused(), precision="bf16", precision_schedule="bf16:3,f16x3", **form)
        with pytest.raises(NotImplementedError, match="canvas_group"):
            fn(_Sharded(), precision_schedule="bf16:3,f16x3", **form)
        with pytest.raises(ValueError, match="precision_log"):
            fn(_Unused(), precision_schedule="bf16:3,f16x3", precision_log=(), **form)
    edm = inspect.unwrap(MODEL.ConditionalElucidatedDiffusionSR.tiled_sample)
    with pytest.raises(NotImplementedError, match="DDPM sampler only"):
        edm(_Unused(), condition_x=cond, precision_schedule="bf16:3,f16x3")
    with pytest.raises(NotImplementedError, match="DDPM sampler only"):
        edm(_Unused(), condition_x=cond, precision_log=[])


def test_the_attribute_on_a_sharded_canvas_and_the_plain_plan():
    plan_of = MODEL.ConditionalContinuousTimeGaussianDiffusionSR._precision_plan
    plain = SimpleNamespace(precision="fp32", precision_schedule=None, canvas_group=None)
    assert plan_of(plain, None, None, 4, 0) == (["fp32"] * 4, ["fp32"])
    assert plan_of(plain, "bf16", None, 4, 0) == (["bf16"] * 4, ["bf16"])
    assert plan_of(plain, None, PS.parse_schedule("bf16:3,f16x3"), 4, 0) == (["bf16"] * 3 + ["f16x3"], ["bf16", "f16x3"])
    assert plan_of(plain, None, PS.parse_schedule("bf16:3,f16x3"), 4, 3) == (["bf16"] * 3 + ["f16x3"], ["f16x3"])
    held = SimpleNamespace(precision="fp32", precision_schedule="bf16,f16x3:1", canvas_group=None)
    assert plan_of(held, None, None, 4, 0) == (["bf16"] * 3 + ["f16x3"], ["bf16", "f16x3"])
    assert plan_of(held, "f16x1", None, 4, 0) == (["f16x1"] * 4, ["f16x1"])            # a call's precision= overrides the attribute
    assert plan_of(held, None, PS.parse_schedule("fp32"), 4, 0) == (["fp32"] * 4, ["fp32"])
    held.canvas_group = object()
    with pytest.raises(NotImplementedError, match="canvas_group"):
        plan_of(held, None, None, 4, 0)
    held.canvas_group, held.precision_schedule = None, "bf16:5,f16x3"
    with pytest.raises(ValueError, match="above the run's 4 steps"):
        plan_of(held, None, None, 4, 0)


def test_the_keywords_of_the_wrappers():
    ddpm, edm = MODEL.ConditionalContinuousTimeGaussianDiffusionSR, MODEL.ConditionalElucidatedDiffusionSR
    for fn in (ddpm.tiled_sample, edm.tiled_sample):
        params = inspect.signature(fn).parameters
        assert params["precision_schedule"].default is None and params["precision_log"].default is None, fn.__qualname__
    assert "precision_schedule" not in inspect.signature(ddpm.sample).parameters          # the un-tiled call does not gain it
    assert "precision_schedule" not in inspect.signature(edm.sample).parameters


# ------------------------------------------------------------------------------------------------ the command line
def _argv(*extra):
    return ["-c", "x", "-m", "w", "--input_dir", "i", "--output_dir", "o", *extra]


def test_the_flag_parses():
    a = INF.parse_args(_argv())
    assert a.precision_schedule is None and not hasattr(a, "precision_plan") and a.precision == "f16x3"
    a = INF.parse_args(_argv("--precision_schedule", "bf16:40,f16x3", "--num_sample_steps", "50"))
    assert a.precision_schedule == "bf16:40,f16x3" and a.precision_plan == ["bf16"] * 40 + ["f16x3"] * 10
    a = INF.parse_args(_argv("--precision_schedule", "bf16,f16x3:10"))                    # 250 steps by default
    assert a.precision_plan == ["bf16"] * 240 + ["f16x3"] * 10


@pytest.mark.parametrize("spec,token", BAD_SPECS + [("bf16:300,f16x3", "above the run's 250 steps"), ("bf16:40,f16x3:10", "sum to 50")],
                         ids=lambda v: repr(v))
def test_a_bad_spec_ends_the_run_before_the_model_is_built(spec, token, monkeypatch):
    def built(*a, **k):
        raise AssertionError("the model was built")
    monkeypatch.setattr(INF, "get_model", built)
    monkeypatch.setattr(INF, "load_config", built)
    with pytest.raises(SystemExit) as err:
        INF.main(_argv(f"--precision_schedule={spec}"))
    assert "--precision_schedule" in str(err.value) and token in str(err.value)


class _Net:
    def __init__(self):
        self.packed = []

    def engine(self, precision, lane=0):
        self.packed.append((precision, lane))


class _Wrapper:
    """What ``main`` needs of a built model: the engine knobs it sets and the U-Net whose engines it packs."""

    def __init__(self):
        self.model, self.step_lanes, self.precision, self.precision_schedule, self.noise_source = _Net(), None, "fp32", None, "host"
        self.module = self

    def eval(self):
        return self

    def to(self, device):
        return self

    def state_dict(self):
        return {}


def _main(monkeypatch, capsys, *flags, model="conditional_continuous"):
    """``main`` with the model, the GPU and the batch driver replaced: (wrapper, the driver's arguments, what was printed)."""
    wrapper, handed = _Wrapper(), []

    def built(conf, logger):
        assert model == "conditional_continuous", "the model was built"
        return wrapper
    monkeypatch.setattr(INF, "load_config", lambda path: SimpleNamespace(model=model, num_classes=3))
    monkeypatch.setattr(INF, "get_model", built)
    monkeypatch.setattr(INF, "batch_sr_target_images", lambda *a, **k: handed.append((a, k)))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    INF.main(_argv("--num_sample_steps", "50", *flags))
    assert len(handed) == 1
    return wrapper, handed[0], capsys.readouterr().out


def test_what_the_command_line_hands_on(monkeypatch, capsys):
    plain, (args0, kw0), out0 = _main(monkeypatch, capsys, "--precision", "bf16")
    assert plain.precision == "bf16" and plain.precision_schedule is None
    assert plain.model.packed == [("bf16", 0), ("bf16", 1)]
    assert "engine precision: bf16 (noise: host)" in out0 and "schedule" not in out0.split("Namespace(")[0]
    assert args0 == ("i", "o", plain) and not any("precision" in k for k in kw0)
    mixed, (args1, kw1), out1 = _main(monkeypatch, capsys, "--precision_schedule", "bf16:40,f16x3", "--device_noise")
    assert mixed.precision_schedule == "bf16:40,f16x3"
    assert mixed.model.packed == [("bf16", 0), ("bf16", 1), ("f16x3", 0), ("f16x3", 1)]
    assert "engine precision schedule: bf16 x40, f16x3 x10 (noise: device)" in out1 and "engine precision: " not in out1
    # the attribute carries the schedule: the batch driver gets the keywords it gets without the flag, and the same values
    assert args1[:2] == args0[:2] and kw1 == kw0
    # the engines of steps that are not run are not packed; fp32 keeps one lane
    late, _, _ = _main(monkeypatch, capsys, "--precision_schedule", "bf16:40,fp32", "--generation_start_steps", "45")
    assert late.model.packed == [("fp32", 0)]
    full, _, _ = _main(monkeypatch, capsys, "--precision_schedule", "bf16:50,f16x3")
    assert full.model.packed == [("bf16", 0), ("bf16", 1)]


def test_an_edm_config_ends_the_run_before_the_model_is_built(monkeypatch, capsys):
    with pytest.raises(SystemExit, match="--precision_schedule: .*EDM"):
        _main(monkeypatch, capsys, "--precision_schedule", "bf16:40,f16x3", model="conditional_elucidated")
