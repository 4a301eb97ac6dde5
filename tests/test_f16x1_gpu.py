"""GPU tests of the f16x1 precision (SRGD_PRECISION_F16X1): the one-term instances of conv3x3_split_kernel through the kernel-level C
ABI (impl 16, impl 17 = with the producer's GroupNorm + SiLU applied in staging) against the mode's definition
    y = conv(hi(x), hi(w s)) / s + bias                       (tests/test_f16x1_cpu.py: emu1)
and the engine mode against the reference's fixtures, the f16x3 engine and the bf16 engine.  The mode is a THROUGHPUT mode: nothing
here holds it to the 1e-3 parity bar."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.split_emulation import split_conv2d, weight_scale
from tests.golden import cases as GC
from tests.test_f16x1_cpu import SHAPES, emu1, seed11_inputs
from tests.test_kernels_gpu import DEV, L, _report_k, ptr, run_conv, stream, to_dev_nhwc

pytestmark = pytest.mark.gpu


def conv64(x, w, b, **kw):
    return F.conv2d(x.double(), w.double(), None if b is None else b.double(), **kw)


def conv1(x, w, b, impl=16, **kw):
    return run_conv(x, None, w, b, ks=3, stride=1, pad=1, kind=0, bf16=False, impl=impl, **kw)


@pytest.mark.parametrize("cfg", SHAPES, ids=lambda s: "B%d_C%d+%d_Cout%d_%dx%d" % s)
def test_one_term_kernel_computes_its_definition(cfg):
    B = cfg[0]
    x0, x1, w, b = seed11_inputs(cfg)
    xin = x0 if x1 is None else torch.cat((x0, x1), 1)
    scale = max(1.0, float(conv64(xin, w, b, padding=1).abs().max()))
    got, part = run_conv(x0, x1, w, b, ks=3, stride=1, pad=1, kind=0, bf16=False, groups=8, impl=16)
    d1 = float((got - emu1(xin, w, b)).abs().max())
    d3 = float((got - split_conv2d(xin, w, b, padding=1, terms=3)).abs().max())
    print("f16x1 kernel", cfg, "vs emu1", d1, "vs emu3", d3, "scale", scale)
    assert d1 <= 4e-6 * scale, (d1, scale)                    # summation order only
    assert d3 >= 10 * 4e-6 * scale, (d3, scale)               # and it is NOT the three-term arithmetic
    assert torch.isfinite(part).all()
    s = part.sum(2).cpu().double()
    g64 = got.double()
    want_s1, want_s2 = g64.reshape(B, 8, -1).sum(-1), (g64 ** 2).reshape(B, 8, -1).sum(-1)
    assert (s[..., 0] - want_s1).abs().max() <= 1e-4 * max(1.0, float(want_s1.abs().max()))
    assert (s[..., 1] - want_s2).abs().max() <= 1e-4 * float(want_s2.abs().max())


def flip_allowance(t64, act32, w):
    """Per output, what the kernel's own evaluation of silu may move the ONE-term result by.  The kernel computes t = fma(a, x, b) in
    fp32 (half an ulp of t, which silu passes on with the condition number |1 + t (1 - sigmoid(t))| <= 1 + |t|), then v_exp_f32,
    an addition, v_rcp_f32 and a multiplication (1 + 1/2 + 1 + 1/2 ulp), and the reference below is float64 rounded to fp32 (1/2):
    an activation differs from the reference's by at most delta = (4 + |t|) * 2^-23 of its value.  hi() maps both to the SAME f16
    value - and then every product and the result's definition are identical - unless the reference's value lies within delta of
    an f16 rounding boundary; there hi() may move by one f16 ulp, which costs |hi(w s) / s| * ulp at each tap that reads it.  The
    three-term arithmetic has no such term: its lo half carries the difference."""
    from oracle.split_emulation import halves
    hi = act32.half().float()
    m, e = torch.frexp(hi)
    ulp = torch.where(hi == 0, torch.full_like(hi, 2.0 ** -24), torch.ldexp(torch.ones_like(hi), e - 11).clamp_min(2.0 ** -24))
    d = (act32 - hi).abs()
    room = ulp / 2 - d                                            # distance to the nearest rounding boundary
    below_pow2 = (m.abs() == 0.5) & (act32.abs() < hi.abs())      # just below a power of two the spacing is half
    room = torch.where(below_pow2, ulp / 4 - d, room)
    fragile = room <= (4 + t64.abs().float()) * 2.0 ** -23 * act32.abs()
    s = weight_scale(w, "f16")
    return F.conv2d(fragile.float() * ulp, (halves(w * s, "f16")[0] / s).abs(), padding=1), float(fragile.float().mean())


@pytest.mark.parametrize("cfg", [(2, 64, 128, 16, 32), (3, 32, 128, 8, 32)], ids=lambda s: "B%d_C%d_Cout%d_%dx%d" % s)
def test_one_term_kernel_with_groupnorm_in_staging(cfg):
    # the coefficients of test_conv3x3_split_groupnorm_in_staging.  cb != 0: silu(cb) != 0 would leak into the halo if the padding
    # were applied before the activation (the reference pads the ACTIVATED tensor with zeros)
    B, cin, cout, H, W = cfg
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, cin, H, W, generator=g) * 2
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g)
    ca = 1 + 0.3 * torch.randn(B, cin, generator=g)
    cb = 0.5 * torch.randn(B, cin, generator=g)
    coef = torch.stack([ca, cb]).contiguous().to(DEV)
    t64 = ca.double()[:, :, None, None] * x.double() + cb.double()[:, :, None, None]
    act64 = F.silu(t64)
    act = act64.float()
    want = emu1(act, w, b)
    scale = max(1.0, float(F.conv2d(act64, w.double(), b.double(), padding=1).abs().max()))
    # 6e-6 * scale: that test's bound (summation order, against float64) + what it lets v_exp / v_rcp cost, which in this arithmetic
    # is flip_allowance (per output; zero where no operand sits on a rounding boundary)
    allow, frac = flip_allowance(t64, act, w)
    got, part = run_conv(x, None, w, b, ks=3, stride=1, pad=1, kind=0, bf16=False, groups=8, impl=17, gn_tail=(None, coef[0], coef[1]))
    err = (got - want).abs()
    # (measured on the MI355X: 0.2 % of the operands are fragile; 0.34 % / 0 % of the outputs of the two cases pass the base bound, the
    # worst of them by 0.82 of its allowance; outputs without a fragile operand stay within 2.9e-6)
    # how much of the allowance is used: the outputs beyond the base bound, the largest share of its allowance such an output takes, and
    # the worst error over an output WITHOUT a fragile operand (held to the base bound alone)
    over = err > 6e-6 * scale
    used = float(((err - 6e-6 * scale) / allow.clamp_min(1e-30))[over].max()) if bool(over.any()) else 0.0
    clean = float(err[allow == 0].max()) if bool((allow == 0).any()) else float("nan")
    _report_k(test="f16x1_gnin", cfg=list(cfg), max_abs=float(err.max()), base_bound=6e-6 * scale, max_allowance=float(allow.max()),
              mean_allowance=float(allow.mean()), fragile_operand_fraction=frac, outputs_over_base_bound=float(over.float().mean()),
              largest_share_of_allowance_used=used, max_abs_where_no_allowance=clean, worst_excess=float((err - allow).max()))
    assert torch.isfinite(got).all()
    assert bool((err <= 6e-6 * scale + allow).all()), float((err - allow).max())
    s = part.sum(2).cpu().double()
    assert (s[..., 0] - got.double().reshape(B, 8, -1).sum(-1)).abs().max() <= 1e-4 * max(1.0, float(got.abs().sum(1).max()))


def test_one_term_kernel_is_exact_where_nothing_is_dropped():
    # the integers of test_conv3x3_split_integer_exact: hi(x) = x, hi(w s) = w s
    g = torch.Generator().manual_seed(12)
    x = torch.randint(-3, 4, (2, 64, 16, 64), generator=g).float()
    w = torch.randint(-2, 3, (128, 64, 3, 3), generator=g).float()
    b = torch.randint(-4, 5, (128,), generator=g).float()
    assert torch.equal(conv1(x, w, b)[0], F.conv2d(x, w, b, padding=1))
    # impl 17 with coefficients under which silu is the identity in fp32: a = 1, b = 40 (1 + exp(-37) == 1, so silu(v) = v for
    # v = x + 40 in [37, 43]); the padding stays zero, every sum stays far below 2^24
    coef = torch.stack([torch.ones(2, 64), torch.full((2, 64), 40.0)]).contiguous().to(DEV)
    got = run_conv(x, None, w, b, ks=3, stride=1, pad=1, kind=0, bf16=False, impl=17, gn_tail=(None, coef[0], coef[1]))[0]
    assert torch.equal(got, F.conv2d(x + 40, w, b, padding=1))
    # pre-rounded operands: x and w s are f16 values, so the hi path loses nothing of its own
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 96, 16, 32, generator=g).half().float()
    w = torch.randn(128, 96, 3, 3, generator=g) / (3 * 96 ** 0.5)
    s = weight_scale(w, "f16")
    w = (w * s).half().float() / s
    b = torch.randn(128, generator=g)
    want64 = conv64(x, w, b, padding=1)
    err = float((conv1(x, w, b)[0].double() - want64).abs().max())
    assert err <= 4e-6 * max(1.0, float(want64.abs().max())), err


@pytest.mark.parametrize("pos", [(3, 17), (0, 0)], ids=["interior", "corner"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_one_term_kernel_nonfinite_footprint(pos, value):
    g = torch.Generator().manual_seed(21)
    x = torch.randn(1, 64, 8, 32, generator=g)
    w = torch.randn(128, 64, 3, 3, generator=g) / 24
    b = torch.randn(128, generator=g)
    clean = conv1(x, w, b)[0]
    assert torch.isfinite(clean).all()
    y, xx = pos
    x[0, 5, y, xx] = value
    got = conv1(x, w, b)[0]
    foot = torch.zeros(1, 128, 8, 32, dtype=torch.bool)
    foot[:, :, max(0, y - 1):y + 2, max(0, xx - 1):xx + 2] = True
    assert torch.isnan(got[foot]).all()
    assert torch.equal(got[~foot].view(torch.int32), clean[~foot].view(torch.int32))


def test_one_term_kernel_saturates_a_finite_value_beyond_f16():
    g = torch.Generator().manual_seed(22)
    x = torch.randn(1, 64, 8, 32, generator=g)
    w = torch.randn(128, 64, 3, 3, generator=g) / 24
    x[0, 0, 0, 0] = 1e6
    assert torch.isfinite(conv1(x, w, None)[0]).all()


def test_one_term_impls_refuse_what_they_do_not_cover():
    lib = L().lib()

    def call(x, w, impl, bf16=False, ks=3, coef=None):
        B, cin, H, W = x.shape
        d = to_dev_nhwc(x, bf16)
        out = torch.empty(B, H, W, w.shape[0], device=DEV, dtype=d.dtype)
        return lib.srgd_k_conv2d_timed(ptr(d), ptr(None), cin, 0, B, H, W, ks, 1, ks // 2, 0, ptr(w.contiguous().float()), ptr(None),
                                       w.shape[0], ptr(out), ptr(None), ptr(None), 0, int(bf16), impl, 0, None, None, ptr(None),
                                       ptr(None if coef is None else coef[0]), ptr(None if coef is None else coef[1]), stream())

    x, w = torch.randn(1, 64, 8, 32), torch.randn(128, 64, 3, 3) / 24
    assert call(x, w, 16, bf16=True) != 0
    assert call(x, torch.randn(128, 64, 1, 1), 16, ks=1) != 0
    assert call(torch.randn(1, 48, 8, 32), torch.randn(128, 48, 3, 3), 16) != 0
    assert call(x, w, 17) != 0                                   # no coefficients
    assert call(x, w, 16) == 0                                   # and the library is still usable
    torch.cuda.synchronize()


def _psnr(a, b):
    return float(10 * np.log10(1.0 / max(float(((a - b) ** 2).mean()), 1e-20)))


def test_engine_f16x1_sits_between_bf16_and_f16x3_on_the_reference_fixture():
    # dim128_config1, host noise, as test_tiled_sample_bf16_vs_reference_reported runs it.  CPU-priced (profiles/f16x1_numerics.jsonl):
    # 77.46 dB, max-abs 3.81e-3; the gate is this suite's customary 3 dB below.  Random-init weights.
    import os
    from tests.test_engine_gpu import G, _report, build_sampler
    case = next(c for c in GC.SAMPLER_CASES if c["name"] == "dim128_config1")
    want = torch.from_numpy(np.load(os.path.join(G, f"sample_{case['name']}.npz"))["image"])
    sampler = build_sampler(case["dim"], weight_seed=case["weight_seed"])
    cond = GC.sampler_condition(case)
    label = torch.tensor([case["label"]]).cuda()
    sampler.noise_source = "host"
    res = {}
    for prec in ("bf16", "f16x3", "f16x1"):
        torch.manual_seed(case["seed"])
        got = sampler.tiled_sample(batch_size=case["batch_size"], condition_x=cond.cuda(), class_label=label,
                                   num_sample_steps=case["steps"], precision=prec).cpu()
        err = (got - want).abs()
        res[prec] = dict(max_abs=float(err.max()), mean_abs=float(err.mean()), psnr_db=_psnr(got, want))
        _report(test="f16x1_tiled_sample", case=case["name"], precision=prec, **res[prec])
        print("f16x1 engine", prec, res[prec])
        if prec == "f16x1":
            assert torch.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    assert res["f16x1"]["psnr_db"] > 74.4, res
    assert res["f16x1"]["psnr_db"] > res["bf16"]["psnr_db"] + 15, res
    assert res["f16x3"]["max_abs"] < res["f16x1"]["max_abs"] < res["bf16"]["max_abs"], res


def test_engine_f16x1_dispatch():
    from tests.test_engine_gpu import build_sampler
    # Where no layer is eligible for the halo kernel the mode IS f16x3.  That is NOT the dim-16 sampler case dim16_256_cfg1: with
    # dim_mults 1, 2, 4, 8 the deepest stage has 128 channels and, in a 256^2 tile, 32 x 32 pixels - nine 3x3 layers the halo kernel
    # covers (downs.3.3, mid_block1 / 2, ups.0.*), so there the two modes must differ.  The dim-16 U-Net on a 128^2 input
    # (UNET_CASES[0]) has 16 x 16 pixels at that stage: W % 32 != 0, no layer is eligible.
    ucase = next(c for c in GC.UNET_CASES if c["name"] == "dim16_128")
    unet = build_sampler(ucase["dim"], weight_seed=ucase["weight_seed"]).model
    x, cnd, ls = GC.unet_inputs(ucase)
    label, c = GC.unet_mode_args("label_cond", ucase, cnd)
    eps = {}
    try:
        for prec in ("f16x3", "f16x1"):
            unet.precision = prec
            eps[prec] = unet(x.cuda(), ls.cuda(), label.cuda(), c.cuda()).cpu()
    finally:
        unet.precision = "fp32"
    assert torch.isfinite(eps["f16x1"]).all() and torch.equal(eps["f16x1"], eps["f16x3"])
    case = next(c for c in GC.SAMPLER_CASES if c["name"] == "dim16_256_cfg1")
    sampler = build_sampler(case["dim"], weight_seed=case["weight_seed"])
    cond = GC.sampler_condition(case).cuda()
    label = torch.tensor([case["label"]]).cuda()
    sampler.noise_source = "host"
    outs = {}
    for prec in ("f16x3", "f16x1"):
        torch.manual_seed(case["seed"])
        outs[prec] = sampler.tiled_sample(batch_size=case["batch_size"], condition_x=cond, class_label=label,
                                          num_sample_steps=case["steps"], precision=prec).cpu()
    assert torch.isfinite(outs["f16x1"]).all() and not torch.equal(outs["f16x1"], outs["f16x3"])
    # dim 128: two 256^2 conditions in one batch = their solo runs, and so is the list form (--lockstep_tiles)
    sampler = build_sampler(128)
    conds = torch.cat([GC.synthetic_lr_condition(i, 64, 64) for i in range(2)]).cuda()
    label = torch.tensor([0]).cuda()
    sampler.noise_source = "device"
    try:
        sampler.device_noise_seed = 11
        kw = dict(batch_size=8, class_label=label, num_sample_steps=2, precision="f16x1")
        both = sampler.tiled_sample(condition_x=conds, **kw).cpu()
        listed = [o.cpu() for o in sampler.tiled_sample(condition_x=[conds[0:1], conds[1:2]], **kw)]
        x3 = sampler.tiled_sample(condition_x=conds[0:1], **dict(kw, precision="f16x3")).cpu()
        for i in range(2):
            solo = sampler.tiled_sample(condition_x=conds[i:i + 1], **kw).cpu()
            assert torch.equal(both[i:i + 1], solo), i
            assert torch.equal(listed[i], solo), i
        assert torch.isfinite(both).all()
        assert not torch.equal(both[0:1], x3)                    # at dim 128 the one-term kernel does run
    finally:
        sampler.noise_source = "host"


def test_edm_wrapper_f16x1_is_closer_to_f16x3_than_bf16_is():
    # the shortest tiled EDM fixture's geometry (dim16_300x300_zeroinit_noclamp: 3 steps) on the dim-128 U-Net
    from tests.test_engine_gpu import build_edm_sampler
    case = min(GC.EDM_CASES, key=lambda c: c["steps"])
    sampler = build_edm_sampler(128)
    cond = GC.sampler_condition(case).cuda()
    label = torch.tensor([case["label"]]).cuda()
    outs = {}
    for prec in ("f16x3", "f16x1", "bf16"):
        torch.manual_seed(case["seed"])
        outs[prec] = sampler.tiled_sample(batch_size=case["batch_size"], condition_x=cond, class_label=label,
                                          num_sample_steps=case["steps"], precision=prec, **GC.edm_extra_kwargs(case)).cpu()
    assert torch.isfinite(outs["f16x1"]).all()
    e1 = float((outs["f16x1"] - outs["f16x3"]).abs().max())
    eb = float((outs["bf16"] - outs["f16x3"]).abs().max())
    print("f16x1 edm: max-abs vs f16x3", e1, "bf16", eb)
    assert e1 < eb, (e1, eb)
