"""CPU checks of tests/cond_cases.py: the designed network is what it claims, every tolerance comes from the oracle alone, and each
assertion rejects each mutant by a factor of at least 100.

``python -m pytest tests/test_cond_cases_cpu.py -s`` prints every derived tolerance, every mutant's rejection factor, and how far
one forward pass moves under a wrong conditioning row next to the end-to-end gate (cond_cases' module docstring keeps the figures).
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import srgd_oracle as O
from srgd_amd.synth import synth_state_dict
from tests import cond_cases as C
from tests.golden import cases as GC

DIMS = [16, 128]


def test_silu_and_erf_gelu_are_the_identity_or_zero_in_fp32():
    C.assert_devices()


# ------------------------------------------------------------------------------------------------ the designed table
@pytest.mark.parametrize("dim", DIMS)
def test_the_designed_network_touches_the_conditioning_tensors_only(dim):
    sd, base = C.designed_state_dict(dim), synth_state_dict(C.schema(dim), seed=0)
    assert list(sd) == list(base)
    touched = {k for k in sd if not torch.equal(sd[k], base[k])}
    assert touched == {k for k in sd if k.startswith(("model.time_mlp", "model.class_mlp")) or ".mlp.1." in k}
    assert not sd["model.time_mlp.0.weights"].any()
    for k in touched:
        assert torch.equal(sd[k], sd[k].round()) and float(sd[k].abs().max()) < 2.0 ** 24, k
    assert len(C.blocks(dim)) == 19 and sum(2 * c for _, c in C.blocks(dim)) == C.default_layout(dim)[1]


@pytest.mark.parametrize("labels", list(C.LAYOUT_LABELS), ids=str)
@pytest.mark.parametrize("dim", DIMS)
def test_the_designed_table_is_the_integer_restatement_and_names_every_entry(dim, labels):
    sd, ids = C.designed_state_dict(dim), C.LAYOUT_LABELS[labels]
    top = C.designed_trace(sd, dim, C.LAYOUT_LOG_SNR, ids)
    layout, stride = C.default_layout(dim)
    want = C.assemble(C.designed_rows(dim, C.LAYOUT_LOG_SNR, ids), layout, stride)
    print("designed table dim %d %-16s [%d x %d], largest sum of magnitudes %.0f < 2^24" % (dim, labels, want.shape[0], want.shape[1], top))
    assert len(C.LAYOUT_LOG_SNR) >= 3 and float(want.max()) < 2.0 ** 24 and bool((want == want.round()).all())
    # the oracle in fp32 - true erf, true exp - gives the integers bit for bit; in float64 silu(32) is 4e-13 short of 32
    C.assert_exact(C.reference_table(sd, dim, C.LAYOUT_LOG_SNR, ids, torch.float32), want, "oracle fp32")
    assert C.distance(C.reference_table(sd, dim, C.LAYOUT_LOG_SNR, ids, torch.float64), want) <= 1e-6
    with torch.inference_mode():                                          # ... and so do the oracle's own functions
        s = C.strip(sd)
        t = O.time_embedding(s, torch.tensor(C.LAYOUT_LOG_SNR))
        name, cout = C.blocks(dim)[3]
        row = F.linear(F.silu(t + (O.class_embedding(s, torch.tensor([ids[0]])) if ids[0] >= 0 else 0)), s[name + ".mlp.1.weight"], s[name + ".mlp.1.bias"])
        K = len(ids)
        C.assert_exact(row, want[0::K + 1, layout[name][0]:layout[name][0] + 2 * cout], "oracle functions")
    if ids[0] >= 0:
        assert want.unique().numel() == want.numel()                      # no two entries alike: rows, blocks, halves, channels
    else:
        assert torch.equal(want[0::2], want[1::2]) and want[0::2].unique().numel() == want[0::2].numel()       # both rows alike
    # the four fields of an entry are read back
    g = want % C.W_COL
    assert torch.equal(g[0], torch.arange(stride, dtype=torch.float64))


MUTANT_CASES = {"off_by_one_time_row": "K1_label", "label_and_null_rows_swapped": "K1_label", "scale_and_shift_swapped": "K1_label",
                "block_offset_shifted": "K1_label", "class_of_first_label_for_every_k": "K3_out_of_order",
                "silu_after_the_block_linear": "K1_label", "x_feature_dropped": "K1_label"}


@pytest.mark.parametrize("mutant", C.MUTANTS)
@pytest.mark.parametrize("dim", DIMS)
def test_a_wrong_table_misses_by_a_factor_of_100(dim, mutant):
    if mutant == "tanh_gelu":
        s, want, tol = C.gelu_sweep()
        f = C.distance(C.gelu_tanh(s.double()), want) / tol
        print("%-34s gelu sweep (tolerance %.3g): rejected by %.3g" % (mutant, tol, f))
        assert f >= C.MUTANT_FACTOR
        assert C.distance(F.gelu(s), want) <= tol / C.MARGIN + 1e-12 and C.distance(0.5 * s * (1 + torch.erf(s * 0.70710678118654752440)), want) <= tol
    else:
        sd, ids = C.designed_state_dict(dim), C.LAYOUT_LABELS[MUTANT_CASES[mutant]]
        layout, stride = C.default_layout(dim)
        want = C.assemble(C.designed_rows(dim, C.LAYOUT_LOG_SNR, ids), layout, stride)
        wrong = C.reference_table(sd, dim, C.LAYOUT_LOG_SNR, ids, torch.float32, mutant=mutant)
        f = C.exact_factor(wrong, want)
        print("%-34s dim %3d layout %-16s: rejected by %.3g ulp" % (mutant, dim, MUTANT_CASES[mutant], f))
        assert f >= C.MUTANT_FACTOR, (mutant, f)
    for variant in C.VALUE_VARIANTS:                                      # the value tolerance: every mutant but tanh_gelu by 100 as well
        case = C.value_case(dim, variant)
        layout, stride = C.default_layout(dim)
        want = C.assemble(case.want, layout, stride)
        f = C.distance(C.reference_table(C.value_state_dict(dim, variant), dim, case.log_snr, case.class_ids, torch.float64, mutant=mutant), want) / case.tol
        print("%-34s dim %3d values %-20s: rejected by %.3g" % (mutant, dim, variant, f))
        # tanh-GELU: 39.9 to 70 measured, 2e-4 of a value against a few hundred fp32 roundings; its factor of 100 comes from gelu_sweep above
        assert f >= (35 if mutant == "tanh_gelu" else C.MUTANT_FACTOR), (mutant, variant, f)


@pytest.mark.parametrize("variant", C.VALUE_VARIANTS)
@pytest.mark.parametrize("dim", DIMS)
def test_the_value_tolerance_comes_from_the_oracle(dim, variant):
    case = C.value_case(dim, variant)
    top = max(float(v.abs().max()) for v in case.want.values())
    print("values dim %3d %-20s: %d log-SNR values x (3 labels + null), largest |argument| %.0f rad, largest entry %.3g, E32 %.3g, tolerance %.3g" % (
        dim, variant, len(case.log_snr), case.max_arg, top, case.e32, case.tol))
    ls = case.log_snr
    assert ls[:3] == [0.0, 1e-3, -1e-3] and abs(ls[3] - 9.2103) < 1e-4 and abs(ls[4] + 10.0001) < 1e-4 and ls[5:7] == [20.0, -20.0]
    assert len(ls) > 7 and min(ls[7:]) < -1.0 and max(ls[7:]) > 1.0      # the EDM run's 0.25 log(sigma), both ends
    assert case.max_arg > (1000 if variant == "sinusoid_weights_x4" else 250)
    assert case.tol == max(C.MARGIN * case.e32, C.FLOOR_ULPS * C.ulp32(top)) and case.tol <= 64 * C.ulp32(top)
    # the oracle's own functions, in fp32, are the fp32 evaluation the tolerance is taken from
    sd = C.strip(C.value_state_dict(dim, variant))
    with torch.inference_mode():
        t = O.time_embedding(sd, torch.tensor(ls)) + O.class_embedding(sd, torch.tensor([case.class_ids[1]]))
        name, cout = C.blocks(dim)[0]
        e = F.linear(F.silu(t), sd[name + ".mlp.1.weight"], sd[name + ".mlp.1.bias"])
    assert C.distance(e, case.want[name][1::4]) <= case.tol / C.MARGIN * 2


# ------------------------------------------------------------------------------------------------ raw launchers, row addressing
def test_the_linear_rows_cases_are_integer_exact_and_reject_wrong_indexing():
    worst = {}
    for act in (C.ACT_NONE, C.ACT_GELU, C.ACT_SILU_IN):
        for in_f in C.LIN_IN:
            for out_f in C.LIN_OUT:
                for rows in C.LIN_ROWS:
                    for add in C.LIN_ADD:
                        c = C.lin_case(in_f, out_f, rows, add, act)
                        assert c.x_stride > in_f and c.y_stride > out_f and bool(torch.isnan(c.x[:, in_f:]).all())
                        assert torch.equal(c.want, c.want.round())
                        assert C.distance(C.lin_reference(c, in_f, out_f, act), c.want) <= 1e-6, (in_f, out_f, rows, add, act)
                        for m in ("bias_of_the_next_output",) if c.b is not None and out_f > 1 else ():
                            worst[m, act] = max(worst.get((m, act), 0.0), C.exact_factor(C.lin_reference(c, in_f, out_f, act, mutant=m), c.want))
                        if add == "per_row" and rows > 1:
                            worst["add_of_row_0", act] = max(worst.get(("add_of_row_0", act), 0.0),
                                                             C.exact_factor(C.lin_reference(c, in_f, out_f, act, mutant="add_of_row_0"), c.want))
    assert len(worst) == 6
    for (m, act), f in worst.items():
        print("linear_rows act %d mutant %-26s rejected by %.3g ulp" % (act, m, f))
        assert f >= C.MUTANT_FACTOR
    assert {in_f % 64 for in_f in C.LIN_IN} >= {0, 1, 17, 63} and {o % 4 for o in C.LIN_OUT} >= {1, 2, 3}


@pytest.mark.parametrize("half", C.TF_HALF)
def test_the_time_features_cases(half):
    for rows in C.TF_ROWS:
        x, w, want, tol = C.tf_case(half, rows, "zero")
        assert tol == 0.0 and torch.equal(want, torch.cat((x[:, None].double(), torch.zeros(rows, half, dtype=torch.float64), torch.ones(rows, half, dtype=torch.float64)), 1))
        x, w, want, tol = C.tf_case(half, rows, "values")
        arg = float((x[:, None] * w[None] * 2 * C.PI32).abs().max())
        print("time_features half %2d rows %d: largest |argument| %.0f rad, tolerance %.3g" % (half, rows, arg, tol))
        assert tol <= 64 * C.ulp32(1.0) and C.distance(C.time_features_ref(w, x, torch.float32), want) <= tol / C.MARGIN + 1e-12
        # sin <-> cos, and the feature of the next frequency, miss by far more than 100 tolerances
        swapped = torch.cat((want[:, :1], want[:, 1 + half:], want[:, 1:1 + half]), 1)
        assert C.distance(swapped, want) >= C.MUTANT_FACTOR * tol
    assert arg > 100


@pytest.mark.parametrize("C_groups", C.GNC_C, ids=lambda v: "C%d" % v[0])
def test_the_row_addressing_table_names_row_and_column(C_groups):
    Cc, groups = C_groups
    table, stride = C.gnc_table(Cc)
    assert table.unique().numel() == table.numel() and stride == C.GNC_OFFSET + 2 * Cc + C.GNC_PAD and Cc % groups == 0
    assert sorted(C.GNC_ROWS) == list(range(len(C.GNC_ROWS))) and list(C.GNC_ROWS) != sorted(C.GNC_ROWS)
    base = C.gnc_want(Cc, False, 1, 2)
    for step, mul in C.GNC_STEPS:
        for beta1 in (False, True):
            want = C.gnc_want(Cc, beta1, step, mul)
            row = (want[:, 0] - (C.GNC_OFFSET + Cc if not beta1 else 2 * C.GNC_OFFSET + Cc + 1)) / (4096 * (2 if beta1 else 1))
            assert row.tolist() == [r + (0 if step is None else step * mul) for r in C.GNC_ROWS]
    # the neighbouring step's row, the neighbouring sample's row and the other half are 4096, 4096 and C away: ulps of a value < 2^20
    for wrong in (C.gnc_want(Cc, False, 2, 2), C.gnc_want(Cc, False, 1, 2)[[1, 2, 3, 4, 0]], C.gnc_want(Cc, False, 1, 2) - Cc):
        f = C.exact_factor(wrong, base)
        print("gn_coefficients C %3d: a wrong row / half is rejected by %.3g ulp" % (Cc, f))
        assert f >= C.MUTANT_FACTOR


# ------------------------------------------------------------------------------------------------ what the end-to-end gate sees
def test_how_far_a_wrong_conditioning_row_moves_one_forward_pass():
    """Informative: the figures go into cond_cases' docstring; nothing is decided here but that they are finite and visible."""
    case = GC.UNET_CASES[0]
    assert case["name"] == "dim16_128"
    sd = C.strip(synth_state_dict(C.schema(16), seed=case["weight_seed"]))
    cfg = O.UnetCfg(dim=16)
    x, cnd, _ = GC.unet_inputs(case)
    x, cnd = x[:1, :, :64, :64], cnd[:1, :, :64, :64]                     # one sample, a 64 x 64 crop: the conditioning acts per channel
    label = torch.tensor([case["label"]])
    t = 1.0 - torch.arange(51) / 50.0                                     # the 50-step DDPM run's times
    ls = O.log_snr_linear(t)
    swapped = dict(sd)
    for name, cout in C.blocks(16):
        w, b = sd[name + ".mlp.1.weight"], sd[name + ".mlp.1.bias"]
        swapped[name + ".mlp.1.weight"], swapped[name + ".mlp.1.bias"] = torch.cat((w[cout:], w[:cout])), torch.cat((b[cout:], b[:cout]))
    with torch.inference_mode():
        for step in (1, 25, 48):
            eps = O.unet_forward(sd, cfg, x, ls[step:step + 1], label, cnd)
            gate = 1e-4 * max(1.0, float(eps.abs().max()))
            moved = {"neighbouring step's row": C.distance(O.unet_forward(sd, cfg, x, ls[step + 1:step + 2], label, cnd), eps),
                     "label and null rows swapped": C.distance(O.unet_forward(sd, cfg, x, ls[step:step + 1], None, cnd), eps),
                     "scale and shift swapped": C.distance(O.unet_forward(swapped, cfg, x, ls[step:step + 1], label, cnd), eps)}
            for what, d in moved.items():
                print("step %2d of 50 (log-SNR %+.3f): %-28s moves eps by %.3g = %.3g x the gate %.3g" % (step, float(ls[step]), what, d, d / gate, gate))
                assert d > 0 and d < float("inf")


# ------------------------------------------------------------------------------------------------ launch_step_rows
def test_the_step_row_cases_restate_the_formula_and_reject_wrong_rows():
    assert C.step_tile_images(0) == [0, 0, 1, 1, 2, 2] and C.step_tile_images(1) == [0, 1, 2]
    assert C.label_slots([2, 0, 2]) == ([2, 0], [0, 1, 0])
    assert any(first > 0 for first, _ in C.STEP_BATCHES[0]) and any(first > 0 for first, _ in C.STEP_BATCHES[1])
    # the formula by hand: K = 2 (labels 2, 0), EDM second evaluation, two passes of even tiles 4, 5 (image 2, slot 0), null second pass
    assert C.step_rows_want("per_image", 0, 4, 2, 4, 1, 1).tolist() == [3, 3, 5, 5]
    assert C.step_rows_want("per_image", 0, 6, 3, 1, 0, 0).tolist() == [0, 1, 1, 0, 1, 1]           # images 0 1 1: slots 0 1 1, no null pass
    assert C.step_rows_want("one_label", 1, 4, 2, 1, 1, 1).tolist() == [2, 2, 3, 3]
    assert C.step_rows_want("no_label", 0, 4, 2, 0, 0, 0).tolist() == [1, 1, 1, 1]
    seen = {m: 0.0 for m in C.STEP_MUTANTS}
    for mode in C.STEP_LABEL_MODES:
        for launch in C.step_launches(mode, 2):
            want = C.step_rows_want(mode, *launch).float()
            for m in C.STEP_MUTANTS:
                wrong = C.step_rows_want(mode, *launch, mutant=m).float()
                seen[m] = max(seen[m], C.exact_factor(wrong, want) if float(want.max()) > 0 else float((wrong != want).any()) * 1e6)
    for m, f in seen.items():
        print("step rows mutant %-26s rejected by %.3g ulp (integer rows, compared exactly)" % (m, f))
        assert f >= C.MUTANT_FACTOR, (m, f)

