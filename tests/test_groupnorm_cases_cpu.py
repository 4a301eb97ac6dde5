"""Proves tests/groupnorm_cases.py before a GPU sees it: the cases reach the mean-to-std ratios they name, the reference's own
fp32 arithmetic (`e_ref`) stays inside every gate of tests/test_groupnorm_conditioning_gpu.py, and those gates reject the emulated
sum / sum-of-squares statistics exactly where the error model says they must: accepted at R <= 8, rejected at R >= 64 in every
kernel case, rejected at M = 128 in the dim-16 engine case.  A case in which the mutant survived at R >= 64 would be a weak case:
the data are to be fixed, not the gate."""
import functools
import json
import os

import pytest
import torch

from tests import groupnorm_cases as GN

IDS = [s.name for s in GN.ALL]


@functools.lru_cache(maxsize=None)
def _kernel(spec):
    """(case, its convolution output in fp32, the float64 expectation on that output)."""
    c = GN.build(spec)
    y = GN.conv_output(c)
    return c, y, GN.reference(y, spec.groups, c.gamma, c.beta, c.ss, c.res)


def test_the_floor_is_the_existing_groupnorm_tests_tolerance():
    from tests.test_kernels_gpu import tol
    g = torch.Generator().manual_seed(0)
    for scale in (0.3, 1.0, 7.5, 600.0):
        want = scale * torch.randn(64, generator=g)
        for bf16 in (False, True):
            assert GN.floor(bf16, want) == tol(bf16, want, k=2.0)


def test_the_table_covers_every_producer_and_every_channels_per_group_class():
    assert {GN.spec(s, 0, "bias").cpg for s in GN.HALO_SHAPES} == {16, 32, 64, 128}
    assert {i for i, _, _ in GN.PRODUCERS.values()} == {1, 2, 6, 12, 7, 14, None}
    for _, (impl, bf16, shapes) in GN.PRODUCERS.items():
        assert shapes, "a producer without a case"
        for s in shapes:
            b, c0, c1, cout, h, w, groups = GN.SHAPES[s]
            assert cout % groups == 0 and (h * w) % GN.SLOT_PIXELS == 0
            if impl not in (1, 7):                        # the halo kernels: 8 x 32 pixel patches, 32-channel chunks, 128-channel tiles
                assert h % 8 == 0 and w % 32 == 0 and c0 % 32 == 0 and c1 % 32 == 0 and cout % 128 == 0
    assert len({s.name for s in GN.ALL}) == len(GN.ALL)


@pytest.mark.parametrize("spec", GN.ALL, ids=IDS)
def test_cases_reach_their_ratio_in_every_group(spec):
    c, y, _ = _kernel(spec)
    lo, hi = GN.measured_ratio(conv_out := GN.conv_output(c, torch.float64), spec.groups)
    std = conv_out.reshape(spec.B, spec.groups, -1).std(-1, unbiased=False)
    assert 0.5 * GN.SIGMA <= float(std.min()) and float(std.max()) <= 2.0 * GN.SIGMA, (float(std.min()), float(std.max()))
    if spec.ratio == 0:
        assert hi <= 0.5, hi
    else:
        assert 0.5 * spec.ratio <= lo and hi <= 2.0 * spec.ratio, (lo, hi)
    if spec.mode == "data":                                # the mean must not sit in the bias
        assert float(c.bias.abs().max()) < 0.1
    if spec.groups > 1 and spec.ratio:                     # both signs
        m = conv_out.reshape(spec.B, spec.groups, -1).mean(-1)
        assert float(m.min()) < 0 < float(m.max())


@pytest.mark.parametrize("spec", GN.ALL, ids=IDS)
def test_reference_fp32_is_inside_the_gate_and_the_mutant_is_rejected_from_ratio_64(spec):
    c, y, want = _kernel(spec)
    e_ref = GN.err(GN.reference(y, spec.groups, c.gamma, c.beta, c.ss, c.res, dtype=torch.float32), want)
    gate = GN.kernel_gate(e_ref, want)
    assert e_ref <= gate
    e_mut = GN.err(GN.sum_of_squares_mutant(y, spec.groups, c.gamma, c.beta, c.ss, c.res), want)
    print(f"{spec.name}: e_ref {e_ref:.3e}  gate {gate:.3e}  mutant {e_mut:.3e}")
    if spec.ratio <= 8:
        assert e_mut <= gate, (e_mut, gate)
    else:
        assert e_mut > gate, (e_mut, gate)


@pytest.mark.parametrize("shape", list(GN.HALO_SHAPES))
@pytest.mark.parametrize("mode", GN.MODES)
def test_bf16_tensor_cases_reference_is_inside_the_bf16_gate(shape, mode):
    # bf16 tensors are gated at R <= 8 with the existing bf16 tolerance, on the stored (rounded) values: the fp32 reference and the
    # mutant must both be far inside it there - the bf16 gate is about the bf16 store, not about the statistics
    for ratio in GN.BF16_GATED_RATIOS:
        spec = GN.spec(shape, ratio, mode)
        c = GN.build(spec, True)
        y = GN.bf16_round(GN.conv_output(c))
        want = GN.reference(y, spec.groups, c.gamma, c.beta, c.ss, c.res)
        e_ref = GN.err(GN.reference(y, spec.groups, c.gamma, c.beta, c.ss, c.res, dtype=torch.float32), want)
        assert e_ref <= 0.01 * GN.floor(True, want)
        assert torch.isfinite(want).all()


# ---------------------------------------------------------------------------------------------- engine cases
def _schema(dim):
    with open(os.path.join(os.path.dirname(__file__), "golden", f"schema_dim{dim}.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


def test_shifted_state_dict_moves_the_groupnorm_convolutions_biases_alone():
    schema = _schema(16)
    base, a, b = (GN.shifted_state_dict(schema, 0, m) for m in (0, 8, 128))
    moved = [k for k in base if not torch.equal(base[k], b[k])]
    assert moved and all(k.endswith(".proj.bias") for k in moved)
    assert len(moved) == sum(k.endswith(".proj.bias") for k in base)
    for k in moved:
        d8, d128 = (a[k] - base[k]).reshape(8, -1), (b[k] - base[k]).reshape(8, -1)
        assert b[k].dtype == torch.float32
        assert float(d128.abs().max()) <= 128.0 + 1e-3
        assert float((d128 - d128[:, :1]).abs().max()) <= 2e-5            # one constant per group (up to the rounding of bias + offset)
        assert torch.allclose(d128, 16 * d8, atol=1e-4)                   # the same draw, scaled by M
    again = GN.shifted_state_dict(schema, 0, 128)
    assert all(torch.equal(again[k], b[k]) for k in b)


@functools.lru_cache(maxsize=None)
def _engine16(M):
    sd = GN.shifted_state_dict(_schema(16), 0, M)
    x, cnd, ls, label = GN.engine_inputs(16)
    want = GN.oracle_forward(sd, 16, x, cnd, ls, label, torch.float64)
    ref = GN.oracle_forward(sd, 16, x, cnd, ls, label, torch.float32)
    mut = GN.oracle_forward(sd, 16, x, cnd, ls, label, torch.float32, group_norm=GN.mutant_group_norm)
    return want, GN.err(ref, want), GN.err(mut, want)


@pytest.mark.parametrize("M", (0,) + GN.ENGINE_MS)
def test_engine_case_reference_fp32_is_inside_the_gate(M):
    want, e_ref, e_mut = _engine16(M)
    assert torch.isfinite(want).all()
    print(f"dim 16, M = {M}: eps range {float(want.abs().max()):.3f}  e_ref {e_ref:.3e}  mutant {e_mut:.3e}  gate {GN.engine_gate(e_ref, want):.3e}")
    assert e_ref <= GN.engine_gate(e_ref, want)
    assert e_ref <= 1e-4 * max(1.0, float(want.abs().max())), "the fp32 reference itself must sit under the floor up to M = 128"


def test_engine_gate_rejects_the_mutant_at_M_128_and_accepts_it_unshifted():
    want, e_ref, e_mut = _engine16(128)
    assert e_mut > GN.engine_gate(e_ref, want), (e_mut, e_ref)
    want, e_ref, e_mut = _engine16(0)
    assert e_mut <= GN.engine_gate(e_ref, want), (e_mut, e_ref)
