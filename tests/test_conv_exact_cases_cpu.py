"""Proves the table of tests/conv_exact_cases.py before a GPU sees it: every value the exactness argument needs to be an exact
integer is one, in every number format a kernel puts it through, and the assertions of tests/test_conv_exact_gpu.py (torch.equal
on the output, exact equality on the GroupNorm sums) reject each of six subtly wrong convolutions, built on the CPU, in every
case they apply to.  A case in which a mutant survived would be a weak case: the data are to be fixed, not the assertion."""
import pytest
import torch
import torch.nn.functional as F

from oracle import mxfp8 as MX
from oracle.split_emulation import mixed_split_conv2d, split_conv2d
from tests import conv_exact_cases as X

IDS = [s.name for s in X.ALL]
SPLIT_FAMILIES = ("halo", "staging", "generic", "stream")          # run by an f16 / bf16 split-operand kernel (impl 6 - 15)
MX_FAMILIES = ("halo", "staging", "mx3", "stream_mx")              # run by an MX-fp8 kernel (impl 14 / 15: the cross terms)


def _inputs(c):
    return [t for t in (c.x0, c.x1, c.residual) + (c.tail[:1] if c.tail else ()) if t is not None]


def _conv_input(c, dtype):
    """What the convolution itself sums over: the (activated, unshuffled) input, and the padding."""
    s = c.spec
    x = (c.x0 if c.x1 is None else torch.cat((c.x0, c.x1), 1)).to(dtype)
    if s.staging:
        x = c.coef[0].to(dtype)[:, :, None, None] * x + c.coef[1].to(dtype)[:, :, None, None]
    if s.layer == "down":
        x = F.pixel_unshuffle(x, 2)
    return x, (1 if s.layer == "3x3" else 0)


@pytest.mark.parametrize("spec", X.ALL, ids=IDS)
def test_float32_reference_equals_float64_bitwise(spec):
    c = X.build(spec)
    x, pad = _conv_input(c, torch.float32)
    pre32 = F.conv2d(x, c.w, c.bias, padding=pad)
    pre64 = X.reference(c).pre
    assert pre32.dtype == torch.float32 and torch.equal(pre32.double(), pre64)
    assert torch.equal(c.want.float().double(), c.want)


@pytest.mark.parametrize("spec", X.ALL, ids=IDS)
def test_values_are_integers_below_2_24_and_survive_the_tensor_types(spec):
    c = X.build(spec)
    ref = X.reference(c)
    for t in (ref.pre, ref.out):
        assert torch.equal(t, t.round()) and float(t.abs().max()) < X.EXACT_MAX
    # the largest sum of magnitudes any partial accumulation can reach, whatever the order
    x, pad = _conv_input(c, torch.float64)
    bound = F.conv2d(x.abs(), c.w.double().abs(), c.bias.double().abs(), padding=pad)
    assert float(bound.max()) < X.EXACT_MAX
    types = X.FAMILIES[X.family_of(spec)][1]
    for t in _inputs(c):
        assert torch.equal(t, t.round())
        if "bf16" in types:
            assert torch.equal(t.to(torch.bfloat16).float(), t)
        if "fp32" in types and X.family_of(spec) in SPLIT_FAMILIES:
            assert torch.equal(t.to(torch.float16).float(), t)
    if spec.staging:                       # the activated value is what the bf16 / f16 staging rounds
        act, _ = _conv_input(c, torch.float32)
        assert torch.equal(act.to(torch.bfloat16).float(), act) and torch.equal(act.to(torch.float16).float(), act)
        assert (act != 0).all()
    if spec.residual or spec.tail:         # the sum of two bf16-exact integers, exact whichever of the two a bf16 kernel rounds first
        for t in (ref.pre, ref.out):
            assert torch.equal(X.bf16_round(t.float()).double(), t)


@pytest.mark.parametrize("spec", [s for s in X.ALL if X.family_of(s) in MX_FAMILIES], ids=lambda s: s.name)
def test_mx_quantisation_returns_the_input_bitwise(spec):
    c = X.build(spec)
    if not spec.staging:      # (impl 15 quantises the ACTIVATED tensor, 32..36, which e4m3 does not hold: its image only meets w_lo = 0 -
        for x in (c.x0, c.x1):                                       # the emulation below covers that) each source is quantised on its own
            if x is not None:
                nhwc = x.permute(0, 2, 3, 1).contiguous()
                assert torch.equal(MX.quantize(nhwc)[2], nhwc)
    if spec.layer == "down":
        cout, c4 = c.w.shape[:2]
        w4 = c.w.reshape(cout, c4 // 4, 2, 2).permute(0, 2, 3, 1).contiguous()          # [o, p1, p2, c]: one scale per (o, tap, 32 c)
        assert torch.equal(MX.quantize(w4)[2], w4)
    else:
        assert torch.equal(MX.quantize_conv_weight(c.w), c.w)
    if X.family_of(spec) in ("halo", "staging"):                     # impl 14 / 15: f16 leading term + two MX cross terms
        x, pad = _conv_input(c, torch.float32)
        emu = mixed_split_conv2d(x, c.w, c.bias, padding=pad, mode="f16mx2")
        assert torch.equal(emu.double(), X.reference(c).pre)


@pytest.mark.parametrize("spec", [s for s in X.ALL if X.family_of(s) in SPLIT_FAMILIES], ids=lambda s: s.name)
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_split_emulation_reproduces_the_reference_bitwise(spec, kind):
    # the emulation covers the convolution and its bias (not the epilogues): hi halves exact, lo halves zero, the weight scale a power of two
    c = X.build(spec)
    x, pad = _conv_input(c, torch.float32)
    emu = split_conv2d(x, c.w, c.bias, padding=pad, kind=kind)
    assert torch.equal(emu.double(), X.reference(c).pre)


@pytest.mark.parametrize("spec", [s for s in X.ALL if s.staging or s.tail or s.layer == "up"], ids=lambda s: s.name)
def test_silu_is_the_identity_on_every_silu_argument(spec):
    c = X.build(spec)
    a = c.silu_args.float()
    assert torch.equal(a.double(), c.silu_args) and float(a.min()) >= X.SILU_MIN
    assert torch.equal(F.silu(a), a)
    assert torch.equal(a / (1 + torch.exp(-a)), a)                   # the device's precise form, in fp32


def test_every_case_with_a_silu_is_in_the_silu_test():
    for s in X.ALL:
        assert (X.build(s).silu_args is not None) == bool(s.staging or s.tail or s.layer == "up")


@pytest.mark.parametrize("spec", [s for s in X.ALL if s.groups], ids=lambda s: s.name)
def test_statistics_conditions(spec):
    c = X.build(spec)
    assert c.s1.shape == c.s2.shape == (spec.B, spec.groups)
    assert float(c.s2.max()) < X.EXACT_MAX and float(c.s1.abs().max()) < X.EXACT_MAX
    assert torch.equal(c.s1.float().double(), c.s1) and torch.equal(c.s2.float().double(), c.s2)
    # sums differ between the (sample, group) pairs: a slot written to the wrong pair cannot cancel
    assert c.s2.reshape(-1).unique().numel() == c.s2.numel()


@pytest.mark.parametrize("spec", X.ALL, ids=IDS)
def test_every_tap_and_input_channel_has_a_non_zero_weight(spec):
    c = X.build(spec)
    assert (c.w != 0).any(0).all()
    assert 0.0 < c.density <= 1.0 and (c.density == 1.0 or spec.groups)


def test_the_table_is_what_the_kernels_accept():
    # the eligibility rules of the kernel-level ABI (srgd_amd/csrc/kernel_api.hip and the *_eligible functions), restated
    for s in X.HALO + X.STAGING:
        assert s.layer == "3x3" and s.C0 % 32 == 0 and s.C1 % 32 == 0 and s.Cout % 128 == 0 and s.H % 8 == 0 and s.W % 32 == 0
        assert not s.groups or s.Cout // s.groups in (16, 32, 64) or (s.Cout // s.groups) % 128 == 0
    assert all(s.C1 == 0 for s in X.STAGING)
    for s in X.MX3:
        assert s.C0 % 128 == 0 and s.C1 % 128 == 0 and s.Cout % 128 == 0 and s.H % 8 == 0 and s.W % 32 == 0
    for s in X.GENERIC:
        assert s.C0 % 32 == 0 and s.C1 % 32 == 0 and s.Cout % 8 == 0
        assert not s.groups or (128 % (s.Cout // s.groups) == 0 and (s.H * s.W) % 128 == 0)
    for s, unit in [(s, 32) for s in X.STREAM] + [(s, 128) for s in X.STREAM_MX]:
        hw = s.H * s.W // (4 if s.layer == "down" else 1)
        assert s.C0 % unit == 0 and s.C1 % unit == 0 and s.Cout % 128 == 0 and hw % 256 == 0 and not s.groups
        assert s.layer != "up" or (s.Cout // 4) % 128 == 0
        assert not (s.residual and s.tail) and not (s.C1 and s.layer == "down")
    assert max(s.Cout * (s.C0 + s.C1) * s.taps for s in X.ALL) <= 2048 * 384 * 9


# ---------------------------------------------------------------------------------------------- the assertions reject the mutants
def _rounded(t, bf16):
    return X.bf16_round(t.float()) if bf16 else t.float()


@pytest.mark.parametrize("mutant", X.MUTANTS)
def test_the_gpu_assertions_reject_the_mutant_in_every_case_it_applies_to(mutant):
    seen = 0
    for spec in X.ALL:
        if not X.mutant_applies(spec, mutant):
            continue
        seen += 1
        c = X.build(spec)
        m = X.reference(c, mutant)
        if mutant == "stats_skip":
            with pytest.raises(AssertionError, match=r"\(b, group\) = \(%d, %d\)" % (spec.B - 1, spec.groups - 1)):
                X.assert_sums(c, torch.stack((m.s1, m.s2), -1))
            continue
        for elem in X.FAMILIES[X.family_of(spec)][1]:
            with pytest.raises(AssertionError, match="differ from the exact value"):
                X.assert_output(c, _rounded(m.out, elem == "bf16"), elem == "bf16")
    assert seen >= 2, mutant


@pytest.mark.parametrize("spec", X.ALL, ids=IDS)
def test_the_gpu_assertions_accept_the_reference(spec):
    c = X.build(spec)
    for elem in X.FAMILIES[X.family_of(spec)][1]:
        X.assert_output(c, _rounded(c.want, elem == "bf16"), elem == "bf16")
    if spec.groups:
        # the sums as a kernel forms them: fp32 partial slots (here one per output row), added in float64 on the host
        pre = X.reference(c).pre.float().reshape(spec.B, spec.groups, spec.Cout // spec.groups, spec.H, spec.W)
        slots = torch.stack((pre.sum((2, 4)), (pre * pre).sum((2, 4))), -1)           # [B, groups, H, 2] fp32
        assert slots.dtype == torch.float32
        X.assert_sums(c, slots.double().sum(2))
        with pytest.raises(AssertionError, match=r"\(b, group\) = \(0, 0\)"):         # one slot counted twice
            X.assert_sums(c, (slots.sum(2) + slots[:, :, 0] * (torch.arange(spec.B * spec.groups).reshape(spec.B, spec.groups, 1) == 0)).double())
