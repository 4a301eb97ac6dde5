"""Every MX-fp8 quantisation site of the fp8 path against oracle/mxfp8.py, bit for bit, on the cases of tests/mxfp8_cases.py
(tests/test_mxfp8_cases_cpu.py proves the cases and shows that these assertions reject wrong quantisers):

  1  quant_mxfp8                      a designed value sweep, non-finite blocks, every launch branch
  2  gn_apply_silu_mxfp8              an exact family (coefficient map, HOIST lane arithmetic) and a gaussian family against float64
  3  the fused twins, site by site    conv1x1_bf16, conv1x1_mxfp8, conv3x3_mxfp8, gn_apply_silu: twin == MX.quantize(stored tensor)
  4  the host weight quantisers       read back exactly through one-hot convolutions

Every output buffer lies between guard bands (64 bytes for q, 16 for s) that must come back untouched.
"""
import ctypes as C

import pytest
import torch

from oracle import mxfp8 as MX
from tests import mxfp8_cases as M
from tests.test_kernels_gpu import DEV, L, from_dev_nhwc, ptr, run_conv, stream, to_dev_nhwc, tol

pytestmark = pytest.mark.gpu


class Guarded:
    """n payload bytes between two sentinel-filled guard bands; the payload starts out as sentinel too."""

    def __init__(self, n, guard):
        self.n, self.guard = n, guard
        self.buf = torch.full((n + 2 * guard,), M.SENTINEL, dtype=torch.uint8, device=DEV)
        self.view = self.buf[guard: guard + n]

    def check(self, what=""):
        ends = torch.cat([self.buf[: self.guard], self.buf[self.guard + self.n:]]).cpu()
        M.assert_guards(ends, 0, self.guard, what)


def quant_buffers(npix, C):
    return Guarded(npix * C, M.Q_GUARD), Guarded(npix * C // 32, M.S_GUARD)


def run_quant(x_dev, npix, C):
    q, s = quant_buffers(npix, C)
    L().check(L().lib().srgd_k_quant_mxfp8(ptr(x_dev), ptr(q.view), ptr(s.view), npix, C, stream()), "quant")
    torch.cuda.synchronize()
    q.check("q")
    s.check("s")
    return q.view, s.view


# ------------------------------------------------------------------------------------------------ 1. quant_mxfp8
def test_quant_mxfp8_value_sweep_is_bit_exact():
    x, wq, ws = M.sweep()
    q, s = run_quant(x.to(DEV), x.shape[0], 32)
    M.assert_bytes(q.cpu(), s.cpu(), wq, ws, "sweep")


def test_quant_mxfp8_nonfinite_blocks_are_bit_exact():
    x, wq, ws = M.nonfinite()
    q, s = run_quant(x.to(DEV), x.shape[0], 32)
    M.assert_bytes(q.cpu(), s.cpu(), wq, ws, "nonfinite")


@pytest.mark.parametrize("shape", M.LAUNCH_SHAPES, ids=lambda s: "%dx%d" % s)
def test_quant_mxfp8_launch_shapes_are_bit_exact(shape):
    npix, Cc = shape
    base, wq, ws, P = M.launch_case(npix, Cc)
    if P == npix:
        q, s = run_quant(base.to(DEV), npix, Cc)
        M.assert_bytes(q.cpu(), s.cpu(), wq, ws, str(shape))
        return
    idx = torch.arange(npix, device=DEV) % P                 # pixel p holds base[p % P]
    x = base.to(DEV)[idx]
    q, s = run_quant(x, npix, Cc)
    del x
    s_ok = torch.equal(s.reshape(npix, Cc // 32), ws.to(DEV)[idx])
    q_bad = (q.reshape(npix, Cc) != wq.to(DEV)[idx]).any(1)
    if not s_ok or bool(q_bad.any()):                        # report the first wrong pixels with the CPU assertion
        bad = torch.nonzero(q_bad | (s.reshape(npix, Cc // 32) != ws.to(DEV)[idx]).any(1))[:8, 0]
        M.assert_bytes(q.reshape(npix, Cc)[bad].cpu(), s.reshape(npix, Cc // 32)[bad].cpu(), wq[(bad % P).cpu()], ws[(bad % P).cpu()],
                       "%s pixels %s" % (shape, bad.tolist()))
        raise AssertionError("mismatch not reproduced on the CPU")


# ------------------------------------------------------------------------------------------------ 2. gn_apply_silu_mxfp8
def run_gn_quant(case):
    B, hw, Cc = case.x.shape
    q, s = quant_buffers(B * hw, Cc)
    dx, da, db = case.x.to(DEV), case.a.to(DEV), case.b.to(DEV)
    L().check(L().lib().srgd_k_gn_apply_silu_mxfp8(ptr(dx), ptr(q.view), ptr(s.view), ptr(da), ptr(db), B, hw, Cc, stream()), "gn_apply_silu_mxfp8")
    torch.cuda.synchronize()
    q.check("q")
    s.check("s")
    return q.view.cpu(), s.view.cpu()


@pytest.mark.parametrize("shape", M.GN_SHAPES, ids=lambda s: "B%d_hw%d_C%d" % s)
def test_gn_apply_silu_mxfp8_exact_family_is_bit_exact(shape):
    case = M.gn_exact(*shape)
    q, s = run_gn_quant(case)
    M.assert_bytes(q, s, case.q, case.s, "gn exact %s hoist=%s" % (shape, M.gn_launch(*shape).hoist))


@pytest.mark.parametrize("shape", M.GN_SHAPES, ids=lambda s: "B%d_hw%d_C%d" % s)
def test_gn_apply_silu_mxfp8_gaussian_family_matches_float64(shape):
    case = M.gn_gaussian(*shape)
    q, s = run_gn_quant(case)
    und = ~case.elem_decided
    print("undecided elements %d of %d, of which different from the expected byte: %d" %
          (int(und.sum()), und.numel(), int((und & (q.reshape(case.q.shape) != case.q)).sum())))
    M.assert_gn_gaussian(q, s, case, "gn gaussian %s" % (shape,))


# ------------------------------------------------------------------------------------------------ 3. the fused twins
def check_twin(q, s, out_dev, what):
    """q, s: Guarded; out_dev: the stored bf16 NHWC tensor.  -> the expected scale bytes."""
    q.check(what + " q")
    s.check(what + " s")
    stored = out_dev.cpu()
    M.assert_twin(q.view.cpu(), s.view.cpu(), stored, what)
    return MX.quantize(stored.float())[1]


def run_conv_twin(c):
    lib = L().lib()
    if c.window:
        d0, d1 = c.x0.to(DEV).to(torch.bfloat16).contiguous(), None
        B, Hin, Win, _ = c.x0.shape
        C0, C1 = 64, 0
        ps0, wout = c.window
    else:
        d0 = to_dev_nhwc(c.x0, True)
        d1 = None if c.x1 is None else to_dev_nhwc(c.x1, True)
        B, C0, Hin, Win = c.x0.shape
        C1 = 0 if c.x1 is None else c.x1.shape[1]
        ps0, wout = 0, 0
    out = torch.empty(c.out_shape, device=DEV, dtype=torch.bfloat16)
    nq = out.numel()
    q, s = Guarded(nq, M.Q_GUARD), Guarded(nq // 32, M.S_GUARD)
    dres = None if c.residual is None else to_dev_nhwc(c.residual, True)
    tail = [None, None, None]
    if c.gn_tail is not None:
        tail = [to_dev_nhwc(c.gn_tail[0], True), c.gn_tail[1].float().contiguous().to(DEV), c.gn_tail[2].float().contiguous().to(DEV)]
    wh, bh = c.w.contiguous().float(), c.b.contiguous().float()
    kw = c.kw
    L().check(lib.srgd_k_conv2d_twin(ptr(d0), ptr(d1), C0, C1, B, Hin, Win, kw["ks"], kw["stride"], kw["pad"], kw["kind"], ptr(wh),
                                     ptr(bh), c.w.shape[0], ptr(out), ptr(dres), ptr(None), 0, 1, c.impl, None, ptr(tail[0]),
                                     ptr(tail[1]), ptr(tail[2]), ptr(q.view), ptr(s.view), ps0, wout, stream()),
              "srgd_k_conv2d_twin")
    torch.cuda.synchronize()
    return out, q, s


@pytest.mark.parametrize("variant", M.TWIN_VARIANTS_BF16)
def test_conv1x1_bf16_twin_equals_the_quantised_stored_tensor(variant):
    c = M.twin_conv_case(3, variant)
    out, q, s = run_conv_twin(c)
    got = from_dev_nhwc(out)
    assert got.shape == c.want.shape
    assert (got - c.want).abs().max() <= tol(True, c.want, k=2.0)           # the stored tensor is the convolution
    if c.residual is None and c.gn_tail is None:
        print("block-wise error / block maximum: %.3g" % M.assert_stored_blockwise(out.cpu(), c.want.permute(0, 2, 3, 1), variant))
    ws = check_twin(q, s, out, "conv1x1_bf16 " + variant)
    M.assert_scale_diversity(ws, variant)


@pytest.mark.parametrize("variant", M.TWIN_VARIANTS_MX)
def test_conv1x1_mxfp8_twin_equals_the_quantised_stored_tensor(variant):
    c = M.twin_conv_case(4, variant)
    out, q, s = run_conv_twin(c)
    got = from_dev_nhwc(out)
    scale = float(c.want.abs().max())
    assert (got - c.want).abs().max().item() <= 2.0 ** -7 * scale + 1e-5    # as test_conv1x1_mxfp8_matches_the_quantised_reference
    if c.residual is None and c.gn_tail is None:
        print("block-wise error / block maximum: %.3g" % M.assert_stored_blockwise(out.cpu(), c.want.permute(0, 2, 3, 1), variant))
    ws = check_twin(q, s, out, "conv1x1_mxfp8 " + variant)
    M.assert_scale_diversity(ws, variant)


def test_conv2d_twin_refuses_a_kernel_that_writes_no_twin():
    c = M.twin_conv_case(3, "plain")
    c2 = M.TwinConv(c.name, 1, c.x0, c.x1, c.w, c.b, c.kw, want=c.want, out_shape=c.out_shape)      # impl 1: the generic kernel
    with pytest.raises(L().SrgdHipError):
        run_conv_twin(c2)


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "gn_partial"])
@pytest.mark.parametrize("name", [t[0] for t in M.TWIN_3X3])
def test_conv3x3_mxfp8_twin_equals_the_quantised_stored_tensor(name, stats):
    c = M.twin_conv3x3_case(name)
    lib = L().lib()
    B, C0, H, W = c.x0.shape
    C1 = 0 if c.x1 is None else c.x1.shape[1]
    cout = c.w.shape[0]
    d0 = to_dev_nhwc(c.x0, True)
    d1 = None if c.x1 is None else to_dev_nhwc(c.x1, True)
    out = torch.empty(B, H, W, cout, dtype=torch.bfloat16, device=DEV)
    q, s = Guarded(out.numel(), M.Q_GUARD), Guarded(out.numel() // 32, M.S_GUARD)
    nslots = C.c_int(0)
    part = torch.zeros(B * c.groups * (H * W // 32) * 2 * max(1, cout // c.groups // 64) + 16, device=DEV) if stats else None
    wh, bh = c.w.contiguous().float(), c.b.contiguous().float()
    L().check(lib.srgd_k_conv3x3_mxfp8_twin(ptr(d0), ptr(d1), C0, C1, B, H, W, ptr(wh), ptr(bh), cout, ptr(out), ptr(part), c.groups,
                                            0, None, C.byref(nslots), ptr(q.view), ptr(s.view), stream()), "conv3x3_mxfp8_twin")
    torch.cuda.synchronize()
    got = from_dev_nhwc(out)
    scale = float(c.want.abs().max())
    assert (got - c.want).abs().max().item() <= 2.0 ** -8 * scale + 1e-5    # as test_conv3x3_mxfp8_matches_the_quantised_reference
    print("block-wise error / block maximum: %.3g" % M.assert_stored_blockwise(out.cpu(), c.want.permute(0, 2, 3, 1), name))
    ws = check_twin(q, s, out, "conv3x3_mxfp8 %s stats=%s" % (name, stats))
    M.assert_scale_diversity(ws, name)
    if stats:                                                # the statistics epilogue shares registers with the twin
        p = part[: B * c.groups * nslots.value * 2].cpu().reshape(B, c.groups, nslots.value, 2).sum(2)
        wsum = c.want.reshape(B, c.groups, -1).sum(-1)
        wsq = (c.want.double() ** 2).reshape(B, c.groups, -1).sum(-1).float()
        assert torch.allclose(p[..., 0], wsum, rtol=2e-3, atol=2e-2 * float(wsq.max()) ** 0.5)
        assert torch.allclose(p[..., 1], wsq, rtol=2e-3)


@pytest.mark.parametrize("cfg", [(B, hw, Cc, r) for (B, hw, Cc) in M.TWIN_GN for r in (True, False)], ids=lambda c: "B%d_hw%d_C%d_res%d" % c)
def test_gn_apply_silu_twin_equals_the_quantised_stored_tensor(cfg):
    B, hw, Cc, with_res = cfg
    c = M.twin_gn_case(B, hw, Cc, with_res)
    dx = c.x.to(DEV)
    dres = None if c.residual is None else c.residual.to(DEV)
    y = torch.empty_like(dx)
    q, s = quant_buffers(B * hw, Cc)
    dg, db, dp = c.gamma.to(DEV), c.beta.to(DEV), c.partial.to(DEV)
    L().check(L().lib().srgd_k_groupnorm_silu_twin(ptr(dx), ptr(y), ptr(dres), ptr(dp), B, hw, Cc, c.groups, ptr(dg), ptr(db), ptr(None),
                                                   1, 1, ptr(q.view), ptr(s.view), stream()), "groupnorm_silu_twin")
    torch.cuda.synchronize()
    assert (y.float().cpu() - c.want).abs().max() <= tol(True, c.want, k=2.0)      # the stored tensor is the GroupNorm + SiLU (+ residual)
    ws = check_twin(q, s, y, "gn_apply_silu %s" % (cfg,))
    M.assert_scale_diversity(ws.reshape(B, 1, hw, Cc // 32), str(cfg))


# ------------------------------------------------------------------------------------------------ 4. host weight quantisers
def conv3x3_mx(x, w_oihw, bias):
    B, Cin, H, W = x.shape
    cout = w_oihw.shape[0]
    d = to_dev_nhwc(x, True)
    out = torch.empty(B, H, W, cout, dtype=torch.bfloat16, device=DEV)
    wh, bh = w_oihw.contiguous().float(), bias.contiguous().float()
    L().check(L().lib().srgd_k_conv3x3_mxfp8(ptr(d), ptr(None), Cin, 0, B, H, W, ptr(wh), ptr(bh), cout, ptr(out), ptr(None), 8, 0, None,
                                             None, stream()), "conv3x3_mxfp8")
    torch.cuda.synchronize()
    return from_dev_nhwc(out)


@pytest.mark.parametrize("kind", ["zero_bias", "integer_bias", "fp32_subnormal_block"])
def test_pack_conv3x3_mxfp8_weights_read_back_bit_exact(kind):
    w, bias, deq = M.weight_case(9, 128, 128, {"zero_bias": 61, "integer_bias": 63, "fp32_subnormal_block": 67}[kind],
                                 int_bias=kind == "integer_bias", with_subnormal=kind == "fp32_subnormal_block")
    x, sites = M.onehot_3x3(128, 8, 32)
    out = conv3x3_mx(x, w.permute(0, 2, 1).reshape(128, 128, 3, 3), bias)
    M.assert_weights_read_back(M.read_back_3x3(out, sites, 128), deq, bias, "pack_conv3x3_mxfp8 " + kind)


@pytest.mark.parametrize("int_bias", [False, True], ids=["zero_bias", "integer_bias"])
def test_pack_conv1x1_mxfp8_weights_read_back_bit_exact(int_bias):
    # 1x1 over two sources (128 + 128): pixel p carries channel p mod 256
    w, bias, deq = M.weight_case(1, 256, 128, 64 if int_bias else 62, int_bias=int_bias)
    H, W = 16, 32
    x = torch.zeros(1, 256, H * W)
    x[0, torch.arange(H * W) % 256, torch.arange(H * W)] = 1.0
    x = x.reshape(1, 256, H, W)
    out, _ = run_conv(x[:, :128].contiguous(), x[:, 128:].contiguous(), w.permute(0, 2, 1).reshape(128, 256, 1, 1), bias, ks=1,
                      stride=1, pad=0, kind=0, bf16=True, impl=4)
    out = out.reshape(128, H * W)
    assert torch.equal(out[:, :256], out[:, 256:])
    M.assert_weights_read_back(out[:, None, :256].contiguous(), deq, bias, "pack_conv1x1_mxfp8 1x1")


def test_pack_conv1x1_mxfp8_tap_major_weights_read_back_bit_exact():
    # 2x2 / stride 2 (Downsample): output pixel P reads tap P % 4 of channel P // 4; the weights quantise tap-major
    w, bias, deq = M.weight_case(4, 128, 128, 65)
    H, W = 16, 32                                             # output size
    x = torch.zeros(1, 128, 2 * H, 2 * W)
    for P in range(H * W):
        tap, c, y, xx = P % 4, P // 4, P // W, P % W
        x[0, c, 2 * y + tap // 2, 2 * xx + tap % 2] = 1.0
    w_oi = w.permute(0, 2, 1).reshape(128, 512, 1, 1)        # reference layout: channel index (c p1 p2)
    out, _ = run_conv(x, None, w_oi, bias, ks=2, stride=2, pad=0, kind=1, bf16=True, impl=4)
    got = out.reshape(128, H * W // 4, 4).permute(0, 2, 1).contiguous()          # [o, tap, c]
    M.assert_weights_read_back(got, deq, bias, "pack_conv1x1_mxfp8 2x2")
