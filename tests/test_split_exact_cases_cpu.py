"""Proves the table of tests/split_exact_cases.py before a GPU sees it: the halves are the designed ones, the absolute sum of
the three terms stays inside the budget, every (tap, input channel) position is covered, every epilogue value is fp32-exact, the
float64 reference equals its own fp32 evaluation under two summation orders, and torch.equal rejects each of eleven subtly wrong
split convolutions, built on the CPU, in every case it applies to.  A case in which a mutant survived would be a weak case: the
data are to be fixed, not the assertion.  Each test prints its case's figures (pytest -s shows them)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import mxfp8 as MX
from oracle.split_emulation import mixed_split_conv2d, split_conv2d
from tests import split_exact_cases as S

CASES = S.all_cases()
IDS = ["%s-%s%s" % (s.name, k, "-x2m10" if sc else "") for s, k, sc, _ in CASES]


def _case(entry):
    return S.build(*entry[:3])


def test_the_budget_is_one_constant_inside_its_limits():
    assert 20 <= S.BUDGET_BITS <= 22
    assert S.budget("f16") == 2.0 ** S.BUDGET_BITS * 2.0 ** -4 and S.budget("bf16") == 2.0 ** S.BUDGET_BITS * 2.0 ** -11


@pytest.mark.parametrize("entry", CASES, ids=IDS)
def test_halves_budget_and_coverage(entry):
    c = _case(entry)
    spec = c.spec
    assert S.halves_are_the_designed_ones(c)
    share = S.abs_sum_share(c)
    assert share < 1.0
    assert S.covered(c)
    x_lo, w_lo = S.lo_share(c)
    assert x_lo > 0.8 and w_lo > 0.8                                  # p, d = 0 one time in seven
    n = S.products_per_output(spec, c.kind)
    per_row = (c.w != 0).reshape(spec.Cout, -1).sum(1)
    assert int(per_row.max()) <= n and int(per_row.min()) >= 1
    assert c.density <= S.budget_density(spec, c.kind) + 1e-9
    if c.kind == "f16" and spec.K >= 576 and not spec.staging:        # the issue's figures: about 0.2 at K = 576, 0.035 at K = 9 * 384
        assert abs(c.density * spec.K - 127) < 4
    if spec.staging:
        assert n == 5
    print("\n%s: density %.4f (%d of K = %d per output), abs-sum share of the budget %.3f, x_lo != 0 %.3f, w_lo != 0 %.3f" % (
        c.name, c.density, n, spec.K, share, x_lo, w_lo))


@pytest.mark.parametrize("entry", CASES, ids=IDS)
def test_every_epilogue_value_is_fp32_exact(entry):
    c = _case(entry)
    spec = c.spec
    ref = S.reference(c)
    t = S.terms(c)
    exact = lambda v: torch.equal(v.float().double(), v)
    assert exact(ref.acc) and exact(ref.acc / t.s)
    for v in (c.bias, c.residual) + (c.tail if c.tail else ()):
        assert v is None or (torch.equal(v, v.round()) and v.dtype == torch.float32)
    assert float(c.bias.abs().max()) <= 4 or spec.layer == "up"
    if c.scaled:
        # acc is the base case's acc times 2^-10; the bias add is the one rounding (module docstring)
        base = S.build(spec, c.kind, False)
        assert torch.equal(ref.acc, S.reference(base).acc * S.X_SCALE)
        assert torch.equal(c.want, S.reference(base).acc / t.s * S.X_SCALE + c.bias.double().view(1, -1, 1, 1))
        assert torch.equal(c.bias, base.bias) and torch.equal(c.w, base.w) and torch.equal(c.x0, base.x0 * S.X_SCALE)
        assert not exact(ref.pre)                                     # (else the case would not need its note)
        if c.kind == "f16":
            assert float(t.xl.abs().max()) < 2.0 ** -14 and float(t.xh.abs().min()) >= 2.0 ** -14      # lo subnormal, hi normal in f16
    else:
        assert exact(ref.pre) and exact(ref.out)                      # acc / s + b, + residual / tail
        # fp32 evaluation of the epilogue, either association
        pre32 = (ref.acc / t.s).float() + c.bias.view(1, -1, 1, 1)
        assert torch.equal(pre32.double(), ref.pre)
        if spec.residual:
            assert torch.equal((pre32 + c.residual).double(), ref.out)
        if spec.tail:
            h, a, b = c.tail
            tl = a[:, :, None, None] * h + b[:, :, None, None]
            assert torch.equal((pre32 + tl).double(), ref.out)
            assert torch.equal(((ref.acc / t.s).float() + (tl + c.bias.view(1, -1, 1, 1))).double(), ref.out)
    if spec.staging:
        assert S.staging_value_is_an_exact_fma(c)


@pytest.mark.parametrize("entry", [e for e in CASES if e[0].staging or e[0].tail or e[0].layer == "up"],
                         ids=lambda e: "%s-%s" % (e[0].name, e[1]))
def test_silu_is_the_identity_on_every_silu_argument(entry):
    c = _case(entry)
    a = c.silu_args.float()
    assert torch.equal(a.double(), c.silu_args) and float(a.min()) >= S.SILU_MIN
    assert torch.equal(F.silu(a), a)
    assert torch.equal(a / (1 + torch.exp(-a)), a)                   # the device's precise form, in fp32
    assert torch.equal(a * (1 / (1 + torch.exp(-a))), a)             # and the rcp form
    assert entry[0].tail or not torch.equal(a, a.round())            # (the tail's data apart) not on integers this time


def test_every_case_with_a_silu_is_in_the_silu_test():
    for e in CASES:
        assert (_case(e).silu_args is not None) == bool(e[0].staging or e[0].tail or e[0].layer == "up")


def _fp32_other_order(c):
    """acc in fp32, the taps and the 32-channel chunks walked backwards, the three terms interleaved hi*lo, hi*hi, lo*hi per step."""
    t = S.terms(c)
    k = t.wh.shape[2]
    xh, xl = (F.pad(v, (t.pad,) * 4) for v in (t.xh, t.xl))
    ho, wo = xh.shape[2] - k + 1, xh.shape[3] - k + 1
    acc = torch.zeros(xh.shape[0], t.wh.shape[0], ho, wo)
    for ky in reversed(range(k)):
        for kx in reversed(range(k)):
            for c0 in reversed(range(0, xh.shape[1], 32)):
                ph, pl = (v[:, c0:c0 + 32, ky:ky + ho, kx:kx + wo] for v in (xh, xl))
                qh, ql = (v[:, c0:c0 + 32, ky, kx] for v in (t.wh, t.wl))
                acc = acc + torch.einsum("bchw,oc->bohw", ph, ql)
                acc = acc + torch.einsum("bchw,oc->bohw", ph, qh)
                acc = acc + torch.einsum("bchw,oc->bohw", pl, qh)
    assert acc.dtype == torch.float32
    return acc


@pytest.mark.parametrize("entry", CASES, ids=IDS)
def test_reference_equals_its_fp32_evaluation_under_two_summation_orders(entry):
    c = _case(entry)
    ref = S.reference(c)
    t = S.terms(c)
    # order 1: the emulation itself (three fp32 convolutions, cross terms first), with its 1 / s and bias
    emu = split_conv2d(t.act, c.w, c.bias, padding=t.pad, kind=c.kind)
    assert emu.dtype == torch.float32
    if c.scaled:
        assert torch.equal(emu, ref.pre.float())
    else:
        assert torch.equal(emu.double(), ref.pre)
    # order 2: tap- and chunk-wise, backwards, interleaved
    assert torch.equal(_fp32_other_order(c).double(), ref.acc)


@pytest.mark.parametrize("entry", [e for e in CASES if e[1] == "f16" and set(e[3]) & set(S.MX_IMPLS)], ids=lambda e: "%s%s" % (e[0].name, "-x2m10" if e[2] else ""))
def test_all_four_halves_survive_mx_quantisation(entry):
    # impl 14 / 15: the cross terms run on MX-fp8 images of x_hi, x - x_hi, w_hi and w_lo
    c = _case(entry)
    t = S.terms(c)
    nhwc = lambda v: v.permute(0, 2, 3, 1).contiguous()
    c0 = c.spec.C0
    for v in (t.xh, t.act - t.xh):
        for src in ((v[:, :c0], v[:, c0:]) if c.spec.C1 else (v,)):   # each source is quantised on its own
            assert torch.equal(MX.quantize(nhwc(src))[2], nhwc(src))
    assert torch.equal(t.act - t.xh, t.xl)
    for v in (t.wh, t.wl):
        assert torch.equal(MX.quantize_conv_weight(v), v)
    emu = mixed_split_conv2d(t.act, c.w, c.bias, padding=t.pad, mode="f16mx2")
    assert torch.equal(emu, S.reference(c).pre.float())


@pytest.mark.parametrize("entry", CASES, ids=IDS)
def test_torch_equal_rejects_every_mutant_and_accepts_the_reference(entry):
    c = _case(entry)
    S.assert_output(c, S.reference(c).out.float())                    # the reference passes the assertion the mutants must fail
    t = S.terms(c)
    no_lo = (t.hh / t.s + c.bias.double().view(1, -1, 1, 1))
    moved_by_lo = S.moved(no_lo, S.reference(c).pre)
    assert moved_by_lo > 0.9
    line = ["lo terms move %.3f" % moved_by_lo]
    for mutant in S.MUTANTS:
        if not S.mutant_applies(c, mutant):
            continue
        m = S.reference(c, mutant)
        share = S.moved(m.out, c.want)
        line.append("%s %.3f" % (mutant, share))
        assert share > 0.0, (c.name, mutant)
        with pytest.raises(AssertionError, match="differ from the exact value"):
            S.assert_output(c, m.out.float())
    print("\n%s: share of outputs moved: %s" % (c.name, "; ".join(line)))


def test_every_mutant_is_applied_somewhere():
    for mutant in S.MUTANTS:
        assert sum(S.mutant_applies(_case(e), mutant) for e in CASES) >= 2, mutant
    with pytest.raises(ValueError):
        S.reference(_case(CASES[0]), "no_such_mutant")


def test_the_table_is_the_one_asked_for():
    assert [s.name for s in S.HALO] == ["halo_cpg16_one_patch", "halo_cpg32_two_sources", "halo_cpg16_B3", "halo_cpg128"]
    assert S.HALO[3].C0 + S.HALO[3].C1 == 384 and S.HALO[3].Cout == 8 * 128
    assert S.STAGING == S.X.STAGING and S.GENERIC == S.X.GENERIC and S.STREAM == S.X.STREAM
    assert [i for i, _ in S.HALO_IMPLS] == [6, 8, 12, 14] and [i for i, _ in S.STAGING_IMPLS] == [11, 13, 15]
    assert S.GENERIC_IMPLS == [(7, "f16"), (9, "bf16")] and S.STREAM_IMPLS == [(10, "f16")]
    assert len(set(IDS)) == len(IDS)
