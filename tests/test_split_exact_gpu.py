"""Bit-exact tests for the lo halves of every split-operand convolution kernel, through the kernel-level C ABI.  The inputs (non-zero
lo halves in both operands, every partial sum of the three-term arithmetic exact in fp32), their float64 outputs and the assertion
come from tests/split_exact_cases.py (proven in tests/test_split_exact_cases_cpu.py, which also shows that torch.equal rejects a
cross term dropped for one tap of one chunk or for one n-tile, x_lo * w_lo added or put in a cross term's place, x_lo * w_hi added
twice, two lo values exchanged inside an 8-channel piece, the lo image shifted by a halo column, the lo halves of the second source
zeroed, lo taken before the staging activation, 1 / s applied to the bias and f16-subnormal lo values flushed):

  halo       conv3x3_split (impl 6, 8: bf16 halves, 12: the 256-thread form), conv3x3_mx2 (14: the cross terms on MX-fp8 operands):
             one patch, two sources, B = 3, and Cin = 384 with 8 n-tiles (the weight ring wraps)
  staging    the same kernels with GroupNorm-in-staging (impl 11, 13, 15): lo halves of the ACTIVATED values
  generic    conv_igemm_split (7, 9: bf16 halves): 3x3, two sources + residual, a ragged M, 1x1, the 2x2 / stride-2 gather, SiLU + PixelShuffle
  stream     conv1x1_split (10): plain, + residual, + ResnetBlock tail, SiLU + PixelShuffle, the 2x2 / stride-2 gather, a long K walk
  x 2^-10    one halo and one streaming case with every x_lo an f16 subnormal

No tolerance anywhere: torch.equal on the whole output.  A kernel runs once per (case, impl); the cross-kernel test reuses the outputs."""
import functools

import pytest
import torch

from tests import split_exact_cases as S
from tests.test_kernels_gpu import DEV, _report_k, run_conv

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run(spec, kind, impl, scaled=False):
    """The kernel's output as fp32 NCHW on the CPU (no GroupNorm sums: groups = 0).  Cached: nobody may write to the result."""
    c = S.build(spec, kind, scaled)
    kw = dict(spec.run_kw(), bf16=False, impl=impl, groups=0, residual=c.residual)
    if spec.staging:                      # [B][C0] scale and shift in ONE allocation, shift behind scale
        coef = torch.stack(c.coef).contiguous().to(DEV)
        kw["gn_tail"] = (None, coef[0], coef[1])
    elif spec.tail:
        kw["gn_tail"] = c.tail
    return run_conv(c.x0, c.x1, c.w, c.bias, **kw)[0]


def _check(spec, kind, impl, scaled=False):
    c = S.build(spec, kind, scaled)
    got = run(spec, kind, impl, scaled)
    want = S.expected(c)
    if got.shape == want.shape and not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        _report_k(test="split_exact", case=c.name, impl=impl, differing=int(bad.sum()), of=bad.numel(),
                  first=[int(i) for i in bad.nonzero()[0]], max_abs=float((got.double() - c.want)[bad].abs().max()))
    S.assert_output(c, got)


def _params(cases, impls):
    return [pytest.param(s, k, i, id="%s-impl%d-%s" % (s.name, i, k)) for s in cases for i, k in impls]


@pytest.mark.parametrize("spec,kind,impl", _params(S.HALO, S.HALO_IMPLS))
def test_halo_3x3_split_kernels_exact_with_lo_halves(spec, kind, impl):
    _check(spec, kind, impl)


@pytest.mark.parametrize("spec,kind,impl", _params(S.STAGING, S.STAGING_IMPLS))
def test_groupnorm_in_staging_exact_with_lo_halves(spec, kind, impl):
    _check(spec, kind, impl)


@pytest.mark.parametrize("spec,kind,impl", _params(S.GENERIC, S.GENERIC_IMPLS))
def test_generic_split_kernel_exact_with_lo_halves(spec, kind, impl):
    _check(spec, kind, impl)


@pytest.mark.parametrize("spec,kind,impl", _params(S.STREAM, S.STREAM_IMPLS))
def test_streaming_pointwise_split_kernel_exact_with_lo_halves(spec, kind, impl):
    _check(spec, kind, impl)


@pytest.mark.parametrize("spec,kind,impl", [p for s, impls in S.SCALED for p in _params([s], impls)])
def test_f16_subnormal_lo_halves_are_not_flushed(spec, kind, impl):
    _check(spec, kind, impl, True)


def test_halo_forms_and_the_generic_split_kernel_are_bitwise_equal():
    # on these data the summation order cannot matter: stronger than the 3e-6 agreement of tests/test_split_gpu.py
    spec = S.CROSS
    a, b, g = run(spec, "f16", 6), run(spec, "f16", 12), run(spec, "f16", 7)
    S.X.assert_equal_tensors(spec.name, a, b, "impl 6 and impl 12")
    S.X.assert_equal_tensors(spec.name, a, g, "impl 6 and impl 7")
    S.assert_output(S.build(spec, "f16", False), g)
