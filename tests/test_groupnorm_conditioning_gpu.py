"""GroupNorm at large group means, on the GPU: every statistics producer and the whole engine against float64, on the cases of
tests/groupnorm_cases.py (proven in tests/test_groupnorm_cases_cpu.py, which also shows that the gates below reject the plain
sum / sum-of-squares variance from a mean-to-std ratio of 64 and from a bias shift of 128).

Kernel level: a producer's convolution runs once per case; the float64 expectation is taken on the DEVICE's convolution output, so
only the statistics and the apply pass are measured.  fp32-tensor producers are gated at every ratio by
max(4 * e_ref, tol(False, want, k=2.0)), e_ref being torch's fp32 group_norm chain on the same values; bf16-tensor producers by the
existing bf16 tolerance at R <= 8 (beyond, bf16's quantum exceeds the group's spread: finite output, error reported).

Engine level: unet(...) on weights whose GroupNorm convolutions carry a per-group bias of up to +-M, against the float64 oracle on
the same (fp32-rounded) weights: fp32 and f16x3 gated by max(4 * e_ref, 1e-4 * scale), bf16 and f16mx2 reported.

Every figure goes to the parity report (parity_report.jsonl, through tests/test_engine_gpu.py's helper).  Value tests only."""
import ctypes as C
import functools

import pytest
import torch

from tests import groupnorm_cases as GN
from tests.test_engine_gpu import _report, _schema, build_sampler
from tests.test_kernels_gpu import DEV, L, from_dev_nhwc, ptr, run_conv, stream, to_dev_nhwc, tol

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- kernel level
@functools.lru_cache(maxsize=None)
def produce(producer, spec):
    """(convolution output as fp32 NCHW on the CPU, partial slots on the device, slot count).  Cached: read only."""
    impl, bf16, _ = GN.PRODUCERS[producer]
    c = GN.build(spec, bf16)
    if impl is not None:
        y, part, nslots = run_conv(c.x0, c.x1, c.w, c.bias, ks=3, stride=1, pad=1, kind=0, bf16=bf16, groups=spec.groups, impl=impl,
                                   want_slots=True)
    else:
        lib = L().lib()
        d0, d1 = to_dev_nhwc(c.x0, True), (None if c.x1 is None else to_dev_nhwc(c.x1, True))
        out = torch.full((spec.B, spec.H, spec.W, spec.Cout), float("nan"), dtype=torch.bfloat16, device=DEV)
        cap = (spec.H * spec.W // 32) * max(1, spec.cpg // 64)
        part = torch.full((spec.B * spec.groups * cap * 2,), float("nan"), device=DEV)
        w, b = c.w.contiguous(), c.bias.contiguous()
        n = C.c_int(0)
        L().check(lib.srgd_k_conv3x3_mxfp8(ptr(d0), ptr(d1), spec.C0, spec.C1, spec.B, spec.H, spec.W, ptr(w), ptr(b), spec.Cout,
                                           ptr(out), ptr(part), spec.groups, 0, None, C.byref(n), stream()), "srgd_k_conv3x3_mxfp8")
        torch.cuda.synchronize()
        nslots = n.value
        assert 0 < nslots <= cap
        y, part = from_dev_nhwc(out), part[:spec.B * spec.groups * nslots * 2].reshape(spec.B, spec.groups, nslots, 2)
    assert torch.isfinite(part).all(), "the epilogue did not fill every GroupNorm partial slot"
    return y, part.contiguous(), nslots


def groupnorm_on_device(producer, spec):
    _, bf16, _ = GN.PRODUCERS[producer]
    c = GN.build(spec, bf16)
    y, part, nslots = produce(producer, spec)
    d, dres = to_dev_nhwc(y, bf16), to_dev_nhwc(c.res, bf16)
    dg, db, dss = c.gamma.to(DEV), c.beta.to(DEV), c.ss.to(DEV)
    L().check(L().lib().srgd_k_groupnorm_silu(ptr(d), ptr(d), ptr(dres), ptr(part), spec.B, spec.H * spec.W, spec.Cout, spec.groups,
                                              ptr(dg), ptr(db), ptr(dss), nslots, int(bf16), stream()), "groupnorm")
    return c, y, from_dev_nhwc(d)


def _kernel_params(bf16):
    return [pytest.param(p, GN.spec(s, r, m), id="%s-%s" % (p, GN.spec(s, r, m).name))
            for p, (_, b, shapes) in GN.PRODUCERS.items() if b == bf16 for s in shapes for r in GN.RATIOS for m in GN.MODES]


@pytest.mark.parametrize("producer,spec", _kernel_params(False))
def test_fp32_tensor_producers_match_float64_at_every_ratio(producer, spec):
    c, y, got = groupnorm_on_device(producer, spec)
    want = GN.reference(y, spec.groups, c.gamma, c.beta, c.ss, c.res)
    e_ref = GN.err(GN.reference(y, spec.groups, c.gamma, c.beta, c.ss, c.res, dtype=torch.float32), want)
    e = GN.err(got, want)
    gate = max(4.0 * e_ref, tol(False, want, k=2.0))
    assert gate == GN.kernel_gate(e_ref, want)
    lo, hi = GN.measured_ratio(y, spec.groups)
    print(f"{producer} {spec.name}: ratio {lo:.1f}..{hi:.1f}  err {e:.3e}  e_ref {e_ref:.3e}  gate {gate:.3e}")
    _report(test="groupnorm_conditioning_kernel", producer=producer, case=spec.name, max_abs=e, e_ref=e_ref, gate=gate, ratio_max=hi)
    assert torch.isfinite(got).all()
    assert e <= gate, (e, e_ref, gate)


@pytest.mark.parametrize("producer,spec", _kernel_params(True))
def test_bf16_tensor_producers_gated_to_ratio_8_and_finite_beyond(producer, spec):
    c, y, got = groupnorm_on_device(producer, spec)
    want = GN.reference(y, spec.groups, c.gamma, c.beta, c.ss, c.res)
    e = GN.err(got, want)
    gate = tol(True, want, k=2.0)
    print(f"{producer} {spec.name}: err {e:.3e}  bf16 gate {gate:.3e}")
    _report(test="groupnorm_conditioning_kernel", producer=producer, case=spec.name, max_abs=e, gate=gate,
            gated=spec.ratio in GN.BF16_GATED_RATIOS)
    assert torch.isfinite(got).all()
    if spec.ratio in GN.BF16_GATED_RATIOS:
        assert e <= gate, (e, gate)


# ---------------------------------------------------------------------------------------------- engine level
_LOADED = {}


def _unet(dim, M):
    """One sampler per dim; the shifted weights are reloaded only when M changes (the parametrisation walks M outermost per dim)."""
    if dim not in _LOADED:
        _LOADED[dim] = [build_sampler(dim, fresh=True), 0]
    sampler, loaded = _LOADED[dim]
    if loaded != M:
        sampler.load_state_dict(GN.shifted_state_dict(_schema(dim), 0, M), strict=True)
        _LOADED[dim][1] = M
    return sampler.model


@functools.lru_cache(maxsize=None)
def _expectation(dim, M):
    sd = GN.shifted_state_dict(_schema(dim), 0, M)
    x, cnd, ls, label = GN.engine_inputs(dim)
    want = GN.oracle_forward(sd, dim, x, cnd, ls, label, torch.float64)
    e_ref = GN.err(GN.oracle_forward(sd, dim, x, cnd, ls, label, torch.float32), want)
    return want, e_ref


def _forward(unet, precision, x, cnd, ls, label):
    unet.precision = precision
    try:
        got = unet(x.cuda(), ls.cuda(), label.cuda(), cnd.cuda())
        torch.cuda.synchronize()
        return got.cpu()
    finally:
        unet.precision = "fp32"


def _engine_params():
    # (dim outermost, then M: the weights are reloaded six times.)  The two reported precisions run at every M at dim 16; at dim 128,
    # where building an engine of theirs takes 2 - 8 s, at the largest M only.
    return [pytest.param(dim, M, p, id=f"dim{dim}-M{M}-{p}") for dim in GN.ENGINE_DIMS for M in GN.ENGINE_MS
            for p in ("fp32", "f16x3", "bf16", "f16mx2") if p in ("fp32", "f16x3") or dim == 16 or M == max(GN.ENGINE_MS)]


@pytest.mark.parametrize("dim,M,precision", _engine_params())
def test_unet_forward_with_bias_dominated_groups_matches_float64(dim, M, precision):
    want, e_ref = _expectation(dim, M)
    got = _forward(_unet(dim, M), precision, *GN.engine_inputs(dim))
    e = GN.err(got, want)
    gate = GN.engine_gate(e_ref, want)
    gated = precision in ("fp32", "f16x3")
    print(f"dim {dim} M {M} {precision}: err {e:.3e}  e_ref {e_ref:.3e}  gate {gate:.3e}{'' if gated else '  (reported)'}")
    _report(test="groupnorm_conditioning_engine", dim=dim, M=M, precision=precision, max_abs=e, e_ref=e_ref, gate=gate,
            ref_max=float(want.abs().max()), gated=gated)
    assert torch.isfinite(got).all()
    if gated:
        assert e <= gate, (e, e_ref, gate)


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_shifted_forward_at_batch_2_equals_its_batch_1_runs_bitwise(precision):
    unet = _unet(16, 128)
    x, cnd, ls, label = GN.engine_inputs(16, batch=2)
    both = _forward(unet, precision, x, cnd, ls, label)
    for i in range(2):
        solo = _forward(unet, precision, x[i:i + 1], cnd[i:i + 1], ls[i:i + 1], label)
        assert torch.equal(both[i:i + 1], solo), f"sample {i} of the batch differs from its solo run"
