"""Bit-exact integer tests for every convolution kernel path and epilogue, through the kernel-level C ABI.  The inputs, their exact
outputs and GroupNorm sums and the assertions come from tests/conv_exact_cases.py (proven in tests/test_conv_exact_cases_cpu.py,
which also shows that these assertions reject a dropped tap, swapped seam channels, a pixel left out of the sums, padding with
silu(b), a transposed pixel shuffle and swapped coefficient rows):

  halo       conv3x3_bf16 (impl 2), conv3x3_split (6, 8: bf16 halves, 12: the 256-thread form), conv3x3_mx2 (14): every
             channels-per-group class of the register-direct epilogue, two sources, a second n-tile, B = 2 and 3, with the sums
  staging    the same kernels with GroupNorm-in-staging (impl 5, 11, 13, 15): zero padding after the activation, [b][c] coefficients
  mx3        srgd_k_conv3x3_mxfp8, with the sums
  generic    conv_igemm in fp32 and bf16 (impl 1) and with split operands (7, 9): sums, two sources + residual, a ragged M,
             the 2x2 / stride-2 gather, SiLU + PixelShuffle
  stream     conv1x1_bf16 (3), conv1x1_split (10), conv1x1_mxfp8 (4): plain, + residual, + ResnetBlock tail, SiLU + PixelShuffle,
             the 2x2 / stride-2 gather, a long K walk, all at B = 3

No tolerance anywhere: torch.equal on the output (after `.to(bfloat16)` in bf16 mode), exact equality of the slot sums added in
float64.  A kernel runs once per (case, impl); the cross-kernel tests reuse that output."""
import ctypes as C
import functools

import pytest
import torch

from tests import conv_exact_cases as X
from tests.test_kernels_gpu import DEV, L, from_dev_nhwc, ptr, run_conv, stream, to_dev_nhwc

pytestmark = pytest.mark.gpu


def _sums(spec, part, nslots):
    assert 0 < nslots <= X.slot_capacity(spec), f"{spec.name}: {nslots} slots reported, capacity {X.slot_capacity(spec)}"
    assert part.shape == (spec.B, spec.groups, nslots, 2)
    bad = ~torch.isfinite(part).all(-1)
    assert not bad.any(), (f"{spec.name}: {int(bad.sum())} of {bad.numel()} partial slots not written or not finite; first at "
                           f"[b, group, slot] = {bad.nonzero()[0].tolist()}")
    return part.cpu().double().sum(2)


@functools.lru_cache(maxsize=None)
def run(spec, impl, bf16, stats=True):
    """(output as fp32 NCHW on the CPU, slot sums float64 [B, groups, 2] or None).  Cached: nobody may write to the result."""
    c = X.build(spec)
    groups = spec.groups if stats else 0
    kw = dict(spec.run_kw(), bf16=bf16, impl=impl, groups=groups, residual=c.residual, want_slots=True)
    coef = None
    if spec.staging:                      # [B][C0] scale and shift in ONE allocation, shift behind scale
        coef = torch.stack(c.coef).contiguous().to(DEV)
        kw["gn_tail"] = (None, coef[0], coef[1])
    elif spec.tail:
        kw["gn_tail"] = c.tail
    got, part, nslots = run_conv(c.x0, c.x1, c.w, c.bias, **kw)
    return got, (_sums(spec, part, nslots) if groups else None)


@functools.lru_cache(maxsize=None)
def run_mx3(spec):
    c = X.build(spec)
    lib = L().lib()
    d0, d1 = to_dev_nhwc(c.x0, True), (None if c.x1 is None else to_dev_nhwc(c.x1, True))
    out = torch.full((spec.B, spec.H, spec.W, spec.Cout), float("nan"), dtype=torch.bfloat16, device=DEV)
    part = torch.full((spec.B * spec.groups * X.slot_capacity(spec) * 2,), float("nan"), device=DEV)
    w, b = c.w.contiguous(), c.bias.contiguous()
    nslots = C.c_int(0)
    L().check(lib.srgd_k_conv3x3_mxfp8(ptr(d0), ptr(d1), spec.C0, spec.C1, spec.B, spec.H, spec.W, ptr(w), ptr(b), spec.Cout, ptr(out),
                                       ptr(part), spec.groups, 0, None, C.byref(nslots), stream()), "srgd_k_conv3x3_mxfp8")
    torch.cuda.synchronize()
    assert 0 < nslots.value <= X.slot_capacity(spec), (spec.name, nslots.value)
    part = part[:spec.B * spec.groups * nslots.value * 2].reshape(spec.B, spec.groups, nslots.value, 2)
    return from_dev_nhwc(out), _sums(spec, part, nslots.value)


def _check(spec, got, sums, bf16):
    c = X.build(spec)
    X.assert_output(c, got, bf16)
    if spec.groups:
        X.assert_sums(c, sums)


def _params(cases, impls):
    return [pytest.param(s, i, b, id="%s-impl%d-%s" % (s.name, i, "bf16" if b else "fp32")) for s in cases for i, b in impls]


@pytest.mark.parametrize("spec,impl,bf16", _params(X.HALO, X.HALO_IMPLS))
def test_halo_3x3_kernels_exact(spec, impl, bf16):
    _check(spec, *run(spec, impl, bf16), bf16)


@pytest.mark.parametrize("spec", X.HALO, ids=lambda s: s.name)
def test_halo_3x3_bf16_equals_the_generic_kernel(spec):
    # (the generic kernel takes no group of more than 128 channels: it runs without the sums here)
    X.assert_equal_tensors(spec.name, run(spec, 2, True)[0], run(spec, 1, True, False)[0], "impl 2 and impl 1 (bf16)")
    X.assert_output(X.build(spec), run(spec, 1, True, False)[0], True)


@pytest.mark.parametrize("spec", X.HALO, ids=lambda s: s.name)
def test_halo_3x3_split_forms_equal_the_generic_split_kernel(spec):
    a, b, g = run(spec, 6, False)[0], run(spec, 12, False)[0], run(spec, 7, False, False)[0]
    X.assert_equal_tensors(spec.name, a, b, "impl 6 and impl 12")
    X.assert_equal_tensors(spec.name, a, g, "impl 6 and impl 7")
    X.assert_output(X.build(spec), g, False)


@pytest.mark.parametrize("spec,impl,bf16", _params(X.STAGING, X.STAGING_IMPLS))
def test_groupnorm_in_staging_exact(spec, impl, bf16):
    _check(spec, *run(spec, impl, bf16), bf16)


@pytest.mark.parametrize("spec", X.MX3, ids=lambda s: s.name)
def test_conv3x3_mxfp8_exact(spec):
    _check(spec, *run_mx3(spec), True)


@pytest.mark.parametrize("spec,impl,bf16", _params(X.GENERIC, X.GENERIC_IMPLS))
def test_generic_kernel_exact(spec, impl, bf16):
    _check(spec, *run(spec, impl, bf16), bf16)


@pytest.mark.parametrize("spec,impl,bf16", _params(X.STREAM, X.STREAM_IMPLS) + _params(X.STREAM_MX, [(4, True)]))
def test_streaming_pointwise_kernels_exact(spec, impl, bf16):
    _check(spec, *run(spec, impl, bf16), bf16)
