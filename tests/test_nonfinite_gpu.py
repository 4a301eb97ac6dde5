"""Non-finite values must stay visible: NaN / Inf footprint tests, one kernel family at a time, and the same end to end.

The reference clamps with torch.clamp and normalises with F.normalize, which propagate a NaN; a kernel that clamps with
fminf(fmaxf(x, lo), hi), takes fmaxf(norm, eps) or saturates its operands with v_med3 turns the NaN into an ordinary value, and a
diverged step, a corrupt checkpoint or a NaN pixel of the condition image comes out as a plausible finite image.

Kernel level: every case runs its kernel twice on the same seeded inputs - clean, and with ONE poisoned input element - and demands
  (a) the kernel's non-finite mask == ~isfinite(reference(poisoned input)), exactly, in both directions (a kernel that hides the
      value fails, and so does one that poisons more than the operation does);
  (b) everything outside that mask is equal (torch.equal) to the clean run of the same kernel.
The reference is torch's float64 operation or the oracle function the parity test of that kernel uses.  No tolerance enters, with
one exception that the arithmetic forces: an INFINITY in an RMSNorm pixel makes the norm infinite, so F.normalize turns the pixel's
OTHER channels into zeros - finite values that differ from the clean run.  Those elements (reference finite, but not what the clean
reference gives) are compared with the reference at the tolerance of the kernel's own parity test; the mask and the rest of the
tensor are checked as everywhere else.  (b) is at the same time the sharpest check for leaks across tile seams, image borders, the
boundary between batch entries of the flat NHWC buffer and the boundary between two concatenated sources: the poison positions
are chosen to sit on those edges.

Engine level: a NaN pixel of the condition image, or a NaN weight, must give a non-finite image (or an error) in every precision.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import srgd_oracle as O
from tests.test_kernels_gpu import DEV, L, from_dev_nhwc, ptr, rnd, run_conv, stream, to_dev_nhwc, tol

pytestmark = pytest.mark.gpu

VALUES = {"nan": float("nan"), "pinf": float("inf"), "ninf": float("-inf")}


def assert_footprint(got, clean, ref_bad, ref_clean=None, changed_tol=None, whole=False):
    """(a) and (b) of the module docstring.  ``ref_clean`` / ``changed_tol``: the RMSNorm-with-infinity exception.  ``whole``: the
    reference mask may cover the whole tensor (a one-batch-entry case)."""
    mask = ~torch.isfinite(ref_bad)
    assert got.shape == clean.shape == mask.shape
    assert torch.isfinite(clean).all(), "the clean run is not finite"
    assert mask.any(), "the reference does not see the poisoned element: the case tests nothing"
    assert whole or not mask.all(), "the reference mask covers everything: (b) tests nothing"
    got_mask = ~torch.isfinite(got)
    hidden, extra = mask & ~got_mask, got_mask & ~mask
    assert not hidden.any() and not extra.any(), (
        f"non-finite footprint differs from the reference's ({int(mask.sum())} elements): {int(hidden.sum())} hidden "
        f"(first at {hidden.nonzero()[:1].tolist()}), {int(extra.sum())} beyond it (first at {extra.nonzero()[:1].tolist()})")
    keep = ~mask
    if changed_tol is not None:
        changed = keep & (ref_bad != ref_clean)
        keep = keep & ~changed
        if changed.any():
            err = (got[changed].double() - ref_bad[changed].double()).abs().max()
            assert err <= changed_tol, f"finite elements the poison changes in the reference: max|diff| = {float(err):.3e}"
    moved = keep & (got != clean)
    assert torch.equal(got[keep], clean[keep]), (
        f"{int(moved.sum())} elements outside the footprint differ from the clean run (first at {moved.nonzero()[:1].tolist()})")


def conv64(x, w, b, **kw):
    return F.conv2d(x.double(), w.double(), None if b is None else b.double(), **kw)


# ------------------------------------------------------------------ convolutions (srgd_k_conv2d_timed, every impl)
# layer: "3x3" (kind 0, pad 1), "1x1" (kind 0), "down" (kind 1: 2x2 / stride 2), "up" (kind 2: SiLU + PixelShuffle)
# extra: "res" (+ residual), "tail" (+ silu(a * h + b), the ResnetBlock tail in the epilogue), "gnin" (conv(silu(a * x + b)))
# shapes are those of the parity tests of the same kernels (test_kernels_gpu.py, test_split_gpu.py), B >= 2
def _cc(name, impl, bf16, layer, B, c0, c1, cout, H, W, extra=None, seam=None, values=("nan", "pinf", "ninf")):
    return dict(name=name, impl=impl, bf16=bf16, layer=layer, B=B, c0=c0, c1=c1, cout=cout, H=H, W=W, extra=extra, seam=seam, values=values)


HALO_SEAM = ((7, 31), (8, 32))        # the 8 x 32 pixel patches of the 3x3 halo kernels: last pixel of patch (0, 0), first of (1, 1)

CONV_CASES = []
for _dt, _bf in (("fp32", False), ("bf16", True)):
    CONV_CASES += [                                                                   # generic implicit GEMM (conv_igemm.hip)
        _cc(f"igemm_{_dt}_3x3_two_sources_res", 1, _bf, "3x3", 2, 64, 32, 48, 16, 32, "res"),
        _cc(f"igemm_{_dt}_1x1_two_sources", 1, _bf, "1x1", 2, 64, 32, 160, 16, 32),
        _cc(f"igemm_{_dt}_down", 1, _bf, "down", 2, 32, 0, 64, 32, 32),
        _cc(f"igemm_{_dt}_up", 1, _bf, "up", 2, 64, 0, 128, 16, 16),
        _cc(f"igemm_{_dt}_3x3", 1, _bf, "3x3", 2, 32, 0, 64, 16, 16),            # 8 channels per group for the GroupNorm cases below
    ]
CONV_CASES += [
    # bf16 fast paths
    _cc("conv3x3_bf16_two_sources", 2, True, "3x3", 2, 64, 32, 256, 16, 64, seam=HALO_SEAM),
    _cc("conv3x3_bf16_gnin", 5, True, "3x3", 2, 64, 0, 128, 16, 64, "gnin", seam=HALO_SEAM),
    _cc("conv1x1_bf16_two_sources", 3, True, "1x1", 2, 64, 32, 128, 16, 32),
    _cc("conv1x1_bf16_res", 3, True, "1x1", 2, 64, 32, 128, 16, 32, "res"),
    _cc("conv1x1_bf16_tail", 3, True, "1x1", 2, 64, 32, 128, 16, 32, "tail"),
    _cc("conv1x1_bf16_up", 3, True, "up", 2, 64, 0, 512, 16, 32),
    _cc("conv1x1_bf16_down", 3, True, "down", 2, 32, 0, 128, 32, 64),
    # split-operand kernels (fp32 tensors)
    _cc("conv3x3_split_two_sources", 6, False, "3x3", 2, 64, 32, 256, 16, 64, seam=HALO_SEAM),
    _cc("conv3x3_split256_two_sources", 12, False, "3x3", 2, 64, 32, 256, 16, 64, seam=HALO_SEAM),
    _cc("conv3x3_split_gnin", 11, False, "3x3", 2, 64, 0, 128, 16, 64, "gnin", seam=HALO_SEAM),
    _cc("conv3x3_split256_gnin", 13, False, "3x3", 2, 64, 0, 128, 16, 64, "gnin", seam=HALO_SEAM),
    _cc("conv3x3_mx2_two_sources", 14, False, "3x3", 2, 64, 32, 256, 16, 64, seam=HALO_SEAM),
    _cc("conv3x3_mx2_gnin", 15, False, "3x3", 2, 64, 0, 128, 16, 64, "gnin", seam=HALO_SEAM),
    _cc("igemm_split_3x3", 7, False, "3x3", 2, 64, 0, 128, 16, 32),
    _cc("igemm_split_1x1_two_sources", 7, False, "1x1", 2, 96, 32, 192, 16, 24),
    _cc("igemm_split_1x1_res", 7, False, "1x1", 2, 64, 0, 128, 16, 24, "res"),
    _cc("igemm_split_down", 7, False, "down", 2, 64, 0, 128, 32, 48),
    _cc("igemm_split_up", 7, False, "up", 2, 64, 0, 256, 16, 24),
    _cc("conv1x1_split_two_sources", 10, False, "1x1", 2, 96, 32, 256, 16, 32),
    _cc("conv1x1_split_res", 10, False, "1x1", 2, 64, 0, 128, 16, 32, "res"),
    _cc("conv1x1_split_tail", 10, False, "1x1", 2, 64, 0, 128, 16, 32, "tail"),
    _cc("conv1x1_split_up", 10, False, "up", 2, 64, 0, 1024, 16, 32),
    _cc("conv1x1_split_down", 10, False, "down", 2, 64, 0, 128, 32, 32),
    # MX-fp8 pointwise layers: NaN only (an infinity saturating to +-448 is the format's documented rule, tested in
    # test_quant_mxfp8_keeps_a_nan_visible)
    _cc("conv1x1_mxfp8_two_sources", 4, True, "1x1", 2, 128, 128, 128, 16, 32, values=("nan",)),
    _cc("conv1x1_mxfp8_res", 4, True, "1x1", 2, 128, 128, 128, 16, 32, "res", values=("nan",)),
    _cc("conv1x1_mxfp8_tail", 4, True, "1x1", 2, 128, 128, 128, 16, 32, "tail", values=("nan",)),
    _cc("conv1x1_mxfp8_up", 4, True, "up", 2, 128, 0, 512, 16, 32, values=("nan",)),
    _cc("conv1x1_mxfp8_down", 4, True, "down", 2, 128, 0, 128, 32, 64, values=("nan",)),
]
CONV_BY_NAME = {c["name"]: c for c in CONV_CASES}
POSITIONS = ["corner00", "cornerHW", "seam_a", "seam_b", "src0_last", "src1_first"]


def conv_poison_position(cfg, pos):
    """(source, batch entry, channel, y, x) of the poisoned input element, or None where the case has no such position."""
    B, c0, c1, H, W = cfg["B"], cfg["c0"], cfg["c1"], cfg["H"], cfg["W"]
    down = cfg["layer"] == "down"
    if pos == "corner00":            # first element of the buffer; its neighbourhood is clipped at two image borders
        return (0, 0, 0, 0, 0)
    if pos == "cornerHW":            # last pixel of entry 0: the next pixel in memory is entry 1's first row - nothing of it may change
        return (0, 0, c0 // 2, H - 1, W - 1)
    if pos in ("seam_a", "seam_b"):  # the two sides of a seam between two workgroup tiles, in the last batch entry
        if cfg["seam"] is not None:
            y, x = cfg["seam"][pos == "seam_b"]
        else:
            # flat-tiled kernels (128- or 256-row tiles of output pixels): output pixels 255 | 256, or 127 | 128 of a 256-pixel image
            Ho, Wo = (H // 2, W // 2) if down else (H, W)
            edge = 256 if Ho * Wo > 256 else 128
            o = edge - 1 if pos == "seam_a" else edge
            y, x = o // Wo, o % Wo
            if down:                 # the input pixel of that output pixel's 2 x 2 window that lies nearest the seam
                y, x = (2 * y + 1, 2 * x + 1) if pos == "seam_a" else (2 * y, 2 * x)
        return (0, B - 1, 5, y, x)
    if c1 == 0:
        return None
    if pos == "src0_last":           # the boundary between the two concatenated sources of the K walk
        return (0, 1, c0 - 1, H // 2, W // 2 - 1)
    return (1, 1, 0, H // 2 - 1, W // 2)


@functools.lru_cache(maxsize=None)
def conv_inputs(name):
    cfg = CONV_BY_NAME[name]
    B, c0, c1, cout, H, W, bf16, layer, extra = (cfg[k] for k in ("B", "c0", "c1", "cout", "H", "W", "bf16", "layer", "extra"))
    g = torch.Generator().manual_seed(101)
    cin = (c0 + c1) * (4 if layer == "down" else 1)
    ks = 3 if layer == "3x3" else 1
    t = dict(x0=rnd(torch.randn(B, c0, H, W, generator=g), bf16),
             x1=rnd(torch.randn(B, c1, H, W, generator=g), bf16) if c1 else None,
             w=rnd(torch.randn(cout, cin, ks, ks, generator=g) / (ks * cin ** 0.5), bf16 and cfg["impl"] != 4),
             b=torch.randn(cout, generator=g))
    Ho, Wo = (H // 2, W // 2) if layer == "down" else (H, W)
    if extra == "res":
        t["res"] = rnd(torch.randn(B, cout, Ho, Wo, generator=g), bf16)
    if extra == "tail":
        t["h"] = rnd(torch.randn(B, cout, Ho, Wo, generator=g), bf16)
        t["ta"], t["tb"] = 1 + 0.3 * torch.randn(B, cout, generator=g), 0.5 * torch.randn(B, cout, generator=g)
    if extra == "gnin":
        t["ca"], t["cb"] = 1 + 0.3 * torch.randn(B, c0, generator=g), 0.5 * torch.randn(B, c0, generator=g)
    return t


def conv_run(cfg, t, x0, x1, groups=0):
    layer, extra = cfg["layer"], cfg["extra"]
    kw = {"3x3": dict(ks=3, stride=1, pad=1, kind=0), "1x1": dict(ks=1, stride=1, pad=0, kind=0),
          "down": dict(ks=2, stride=2, pad=0, kind=1), "up": dict(ks=1, stride=1, pad=0, kind=2)}[layer]
    gn_tail = None
    if extra == "tail":
        gn_tail = (t["h"], t["ta"], t["tb"])
    if extra == "gnin":
        coef = torch.stack([t["ca"], t["cb"]]).contiguous().to(DEV)        # one allocation, shift behind scale
        gn_tail = (None, coef[0], coef[1])
    return run_conv(x0, x1, t["w"], t["b"], bf16=cfg["bf16"], residual=t.get("res"), impl=cfg["impl"], gn_tail=gn_tail,
                    groups=groups, want_slots=True, **kw)


def conv_reference(cfg, t, x0, x1):
    layer, extra = cfg["layer"], cfg["extra"]
    xin = x0 if x1 is None else torch.cat((x0, x1), 1)
    w, b = t["w"], t["b"]
    if extra == "gnin":
        xin = F.silu(t["ca"].double()[:, :, None, None] * xin.double() + t["cb"].double()[:, :, None, None])
    if layer == "down":
        y = O.space_to_depth_conv({"d.1.weight": w, "d.1.bias": b}, "d", xin).double()
    elif layer == "up":
        y = O.pixel_shuffle_up({"u.net.0.weight": w, "u.net.0.bias": b}, "u", xin).double()
    else:
        y = conv64(xin, w, b, padding=1 if layer == "3x3" else 0)
    if extra == "res":
        y = y + t["res"].double()
    if extra == "tail":
        y = y + F.silu(t["ta"].double()[:, :, None, None] * t["h"].double() + t["tb"].double()[:, :, None, None])
    return y


@functools.lru_cache(maxsize=None)
def conv_clean(name):
    cfg, t = CONV_BY_NAME[name], conv_inputs(name)
    return conv_run(cfg, t, t["x0"], t["x1"])[0]


def poisoned(t, where, value):
    src, b, c, y, x = where
    x0, x1 = t["x0"].clone(), None if t["x1"] is None else t["x1"].clone()
    (x0, x1)[src][b, c, y, x] = value
    return x0, x1


CONV_PARAMS = [pytest.param(c["name"], pos, v, id=f"{c['name']}-{pos}-{v}") for c in CONV_CASES for pos in POSITIONS
               for v in c["values"] if conv_poison_position(c, pos) is not None]


@pytest.mark.parametrize("name,pos,value", CONV_PARAMS)
def test_conv_nonfinite_footprint(name, pos, value):
    cfg, t = CONV_BY_NAME[name], conv_inputs(name)
    x0, x1 = poisoned(t, conv_poison_position(cfg, pos), VALUES[value])
    got = conv_run(cfg, t, x0, x1)[0]
    assert_footprint(got, conv_clean(name), conv_reference(cfg, t, x0, x1))


# ------------------------------------------------------------------ srgd_k_conv3x3_mxfp8 (its own entry point)
@pytest.mark.parametrize("pos", ["corner00", "cornerHW", "seam_a", "seam_b", "src0_last", "src1_first"])
def test_conv3x3_mxfp8_nan_footprint(pos):
    lib = L().lib()
    B, c0, c1, cout, H, W = 2, 128, 256, 256, 16, 64
    cfg = dict(B=B, c0=c0, c1=c1, H=H, W=W, layer="3x3", seam=HALO_SEAM)
    g = torch.Generator().manual_seed(102)
    t = dict(x0=rnd(torch.randn(B, c0, H, W, generator=g), True), x1=rnd(torch.randn(B, c1, H, W, generator=g), True))
    w = torch.randn(cout, c0 + c1, 3, 3, generator=g) / (9 * (c0 + c1)) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)

    def run(x0, x1):
        d0, d1 = to_dev_nhwc(x0, True), to_dev_nhwc(x1, True)
        out = torch.empty(B, H, W, cout, dtype=torch.bfloat16, device=DEV)
        L().check(lib.srgd_k_conv3x3_mxfp8(ptr(d0), ptr(d1), c0, c1, B, H, W, ptr(w), ptr(b), cout, ptr(out), ptr(None), 8, 0, None,
                                           None, stream()), "conv3x3_mxfp8")
        torch.cuda.synchronize()
        return from_dev_nhwc(out)

    x0, x1 = poisoned(t, conv_poison_position(cfg, pos), float("nan"))
    assert_footprint(run(x0, x1), run(t["x0"], t["x1"]), conv64(torch.cat((x0, x1), 1), w, b, padding=1))


# ------------------------------------------------------------------ conv -> GroupNorm partial slots -> srgd_k_groupnorm_silu
GN_CASES = {          # name: (conv case whose shape and kernel are used, groups)
    "igemm_fp32": ("igemm_fp32_3x3", 8), "igemm_bf16": ("igemm_bf16_3x3", 8),
    "conv3x3_bf16": ("conv3x3_bf16_two_sources", 8), "conv3x3_split": ("conv3x3_split_two_sources", 8),
    "conv3x3_split256": ("conv3x3_split256_two_sources", 8), "conv3x3_mx2": ("conv3x3_mx2_two_sources", 8),
    "igemm_split": ("igemm_split_3x3", 8),
}


@pytest.mark.parametrize("pos", ["corner00", "cornerHW", "seam_b"])
@pytest.mark.parametrize("name", list(GN_CASES))
def test_groupnorm_statistics_carry_a_nan_of_the_convolution(name, pos):
    # a NaN output of the convolution must reach its GroupNorm partial slot: every group that holds one comes out NaN as a whole
    # (F.group_norm), and the other batch entries do not move by a bit
    lib = L().lib()
    conv_name, groups = GN_CASES[name]
    cfg, t = dict(CONV_BY_NAME[conv_name], extra=None), conv_inputs(conv_name)
    B, cout, H, W, bf16 = cfg["B"], cfg["cout"], cfg["H"], cfg["W"], cfg["bf16"]
    g = torch.Generator().manual_seed(103)
    gamma, beta = 1 + 0.2 * torch.randn(cout, generator=g), 0.3 * torch.randn(cout, generator=g)
    dg, db_ = gamma.to(DEV), beta.to(DEV)

    def run(x0, x1):
        conv_out, part, nslots = conv_run(cfg, t, x0, x1, groups=groups)
        d = to_dev_nhwc(conv_out, bf16)
        part = part.contiguous()
        L().check(lib.srgd_k_groupnorm_silu(ptr(d), ptr(d), ptr(None), ptr(part), B, H * W, cout, groups, ptr(dg), ptr(db_),
                                            ptr(None), nslots, int(bf16), stream()), "groupnorm")
        torch.cuda.synchronize()
        return from_dev_nhwc(d)

    x0, x1 = poisoned(t, conv_poison_position(cfg, pos), float("nan"))
    ref = F.silu(F.group_norm(conv_reference(cfg, t, x0, x1), groups, gamma.double(), beta.double(), eps=1e-5))
    assert_footprint(run(x0, x1), run(t["x0"], t["x1"]), ref)


# ------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("value", ["nan", "pinf"])
@pytest.mark.parametrize("pos", ["first", "last_of_entry0", "middle"])
@pytest.mark.parametrize("Cc", [16, 128, 1024])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_rmsnorm_nonfinite_footprint(bf16, Cc, pos, value):
    # NaN: the whole pixel (F.normalize divides every channel by the NaN norm).  +Inf: the norm is infinite, the element itself
    # becomes Inf / Inf = NaN and the pixel's other channels 0 (+ residual): one non-finite element, C - 1 changed finite ones
    lib = L().lib()
    g = torch.Generator().manual_seed(6)
    x = rnd(torch.randn(2, Cc, 8, 16, generator=g) * 3, bf16)
    gain = 1 + 0.1 * torch.randn(1, Cc, 1, 1, generator=g)
    res = rnd(torch.randn(2, Cc, 8, 16, generator=g), bf16)
    dgain = gain.reshape(-1).to(DEV)

    def run(xx):
        d, dres = to_dev_nhwc(xx, bf16), to_dev_nhwc(res, bf16)
        out = torch.empty_like(d)
        L().check(lib.srgd_k_rmsnorm(ptr(d), ptr(out), ptr(dres), ptr(dgain), 2 * 8 * 16, Cc, int(bf16), stream()), "rmsnorm")
        torch.cuda.synchronize()
        return from_dev_nhwc(out)

    bad = x.clone()
    b, c, y, xx = {"first": (0, 0, 0, 0), "last_of_entry0": (0, Cc - 1, 7, 15), "middle": (1, Cc // 2, 3, 9)}[pos]
    bad[b, c, y, xx] = VALUES[value]
    ref_clean, ref_bad = O.rms_norm(x, gain) + res, O.rms_norm(bad, gain) + res
    assert_footprint(run(bad), run(x), ref_bad, ref_clean=ref_clean, changed_tol=tol(bf16, ref_clean))
    assert int((~torch.isfinite(ref_bad)).sum()) == (Cc if value == "nan" else 1)


# ------------------------------------------------------------------ conv1x1_split with the RMSNorms folded in
@pytest.mark.parametrize("value", ["nan", "pinf", "ninf"])
@pytest.mark.parametrize("pos", ["first", "last_of_entry0", "seam_a", "seam_b"])
@pytest.mark.parametrize("cfg", [("pre", 128, 384, 2, 512), ("pre", 256, 384, 2, 256), ("pre", 1024, 384, 2, 1024), ("post", 128, 128, 2, 512)],
                         ids=lambda c: "%s_C%d_Cout%d_B%d_N%d" % c)
def test_conv1x1_split_rms_nonfinite_footprint(cfg, pos, value):
    # pre: RMSNorm(x) @ w^T - a non-finite channel makes the pixel's norm non-finite, so all Cout outputs of that pixel;
    # post: RMSNorm(x @ w^T + bias) * g + res - every output of the pixel is non-finite ahead of the norm already
    kind, cin, cout, B, N = cfg
    lib = L().lib()
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, N, cin, generator=g) * torch.logspace(-1, 1, N).view(1, N, 1)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    gain = 1 + 0.3 * torch.randn(cin if kind == "pre" else cout, generator=g)
    bias = None if kind == "pre" else torch.randn(cout, generator=g)
    res = None if kind == "pre" else torch.randn(B, N, cout, generator=g)
    wh, gh = w.contiguous(), gain.contiguous()
    bh = None if bias is None else bias.contiguous()
    dres = None if res is None else res.contiguous().to(DEV)

    def rms64(v, gg):
        v = v.double()
        return v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12) * gg.double() * v.shape[-1] ** 0.5

    def reference(xx):
        if kind == "pre":
            return rms64(xx, gain) @ w.double().t()
        return rms64(xx.double() @ w.double().t() + bias.double(), gain) + res.double()

    def run(xx):
        dx = xx.contiguous().to(DEV)
        out = torch.empty(B, N, cout, device=DEV)
        L().check(lib.srgd_k_conv1x1_split_rms(ptr(dx), cin, B, N, ptr(wh), ptr(bh), cout, ptr(gh if kind == "pre" else None),
                                               ptr(gh if kind == "post" else None), ptr(dres), ptr(out), stream()), "conv1x1_split_rms")
        torch.cuda.synchronize()
        return out.cpu()

    seam = 256 if N > 256 else 128
    b, n, c = {"first": (0, 0, 0), "last_of_entry0": (0, N - 1, cin - 1), "seam_a": (1, seam - 1, 7), "seam_b": (1, seam, cin // 2)}[pos]
    bad = x.clone()
    bad[b, n, c] = VALUES[value]
    assert_footprint(run(bad), run(x), reference(bad))


# ------------------------------------------------------------------ attention cores
ATTN_POISON = {       # name: (tensor 0 / 1 / 2 = q / k / v, batch entry, channel of that tensor, pixel as a fraction of N - 1)
    "q": (0, 0, 37, 0.5),                      # head 1, channel 5: one pixel x the 32 channels of that head
    "k_first_chunk": (1, 1, 2 * 32 + 3, 0.0),  # head 2: every pixel x 32 channels of (batch 1, head 2), from the first chunk of keys
    "k_last_chunk": (1, 0, 127, 1.0),          # head 3, from the last key
    "v": (2, 1, 64, 0.25),                     # every pixel x one channel
}


@pytest.mark.parametrize("poison", list(ATTN_POISON))
@pytest.mark.parametrize("case", [("linear", 16, 16), ("linear", 64, 64), ("linear", 24, 40), ("full", 16, 16), ("full", 32, 32), ("full", 8, 24)],
                         ids=lambda c: "%s_%dx%d" % c)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_attention_core_nan_footprint(bf16, case, poison):
    # the online-softmax kernels merge maxima with fmaxf, which drops a NaN: the NaN score must still reach the sums through
    # exp(s - m) in every path (chunk merge, rescale, the MFMA form), and only the sums the operation feeds with it
    lib = L().lib()
    which, H, W = case
    g = torch.Generator().manual_seed(7 if which == "linear" else 8)
    qkv = torch.randn(2, 384, H, W, generator=g) * (2 if which == "linear" else 1.5)
    if which == "linear":
        qkv[0, 128 + 5, 3, 3] = 9.0
    else:
        qkv[1, :32, 2, 2] *= 6.0
    qkv = rnd(qkv, bf16)
    fn = lib.srgd_k_linear_attention if which == "linear" else lib.srgd_k_full_attention
    core = O.linear_attention_core if which == "linear" else O.full_attention_core

    def run(t):
        d = to_dev_nhwc(t, bf16)
        out = torch.empty(2, H, W, 128, device=DEV, dtype=d.dtype)
        L().check(fn(ptr(d), ptr(out), 2, H * W, 4, int(bf16), stream()), which)
        torch.cuda.synchronize()
        return from_dev_nhwc(out)

    tensor, b, c, frac = ATTN_POISON[poison]
    n = int(round(frac * (H * W - 1)))
    bad = qkv.clone()
    bad[b, tensor * 128 + c, n // W, n % W] = float("nan")
    ref = core(bad, 4, 32)
    assert int((~torch.isfinite(ref)).sum()) == {"q": 32, "k_first_chunk": 32 * H * W, "k_last_chunk": 32 * H * W, "v": H * W}[poison]
    assert_footprint(run(bad), run(qkv), ref)


# ------------------------------------------------------------------ fused linear-attention block
@pytest.mark.parametrize("pos", ["first", "last_of_entry0", "middle_of_last_entry"])
@pytest.mark.parametrize("cfg", [(2, 32, 64), (3, 8, 8), (2, 16, 16)], ids=lambda s: "B%d_%dx%d" % s)
@pytest.mark.parametrize("Cc", [128, 256])
def test_linear_attention_block_fused_nan_footprint(Cc, cfg, pos):
    # RMSNorm -> qkv -> linear attention -> to_out -> RMSNorm -> + x: a NaN pixel of x makes that pixel's k and v NaN, and through
    # the softmax over positions and the context every pixel of that batch entry - and nothing of the others
    B, H, W = cfg
    lib = L().lib()
    g = torch.Generator().manual_seed(21)
    x = rnd(torch.randn(B, Cc, H, W, generator=g) * 1.5, True)
    sd = {"a.norm.g": 1 + 0.1 * torch.randn(1, Cc, 1, 1, generator=g),
          "a.to_qkv.weight": torch.randn(384, Cc, 1, 1, generator=g) / Cc ** 0.5,
          "a.to_out.0.weight": torch.randn(Cc, 128, 1, 1, generator=g) / 128 ** 0.5,
          "a.to_out.0.bias": 0.1 * torch.randn(Cc, generator=g),
          "a.to_out.1.g": 1 + 0.1 * torch.randn(1, Cc, 1, 1, generator=g)}
    hw = [sd["a.to_qkv.weight"].reshape(384, Cc).contiguous(), sd["a.norm.g"].reshape(Cc).contiguous(),
          sd["a.to_out.0.weight"].reshape(Cc, 128).contiguous(), sd["a.to_out.0.bias"].contiguous(),
          sd["a.to_out.1.g"].reshape(Cc).contiguous()]

    def run(t):
        d = to_dev_nhwc(t, True)
        y = torch.empty_like(d)
        L().check(lib.srgd_k_linattn_block_fused(ptr(d), ptr(y), B, H * W, Cc, *[ptr(w_) for w_ in hw], stream()), "fused")
        torch.cuda.synchronize()
        return from_dev_nhwc(y)

    b, c, y_, x_ = {"first": (0, 0, 0, 0), "last_of_entry0": (0, Cc - 1, H - 1, W - 1), "middle_of_last_entry": (B - 1, 70, H // 2, W // 3)}[pos]
    bad = x.clone()
    bad[b, c, y_, x_] = float("nan")
    ref = O.linear_attention(sd, "a", bad, 4, 32) + bad
    assert int((~torch.isfinite(ref)).sum()) == Cc * H * W
    assert_footprint(run(bad), run(x), ref)


# ------------------------------------------------------------------ engine level
# dim 128 (at dim 16 most layers have Cin % 32 != 0 and run on the exact-fp32 kernel in every mode), host noise, 2 steps, one
# 256 x 256 condition image = one tile per step.  The call may raise; a finite image is the failure.
def _cond(seed=0):
    from tests.golden import cases as GC
    return GC.synthetic_lr_condition(seed, 64, 64)            # [1, 3, 256, 256] in [0, 1]


def _poison_pixel(cond):
    cond = cond.clone()
    cond[0, 1, 100, 141] = float("nan")
    return cond


def _nonfinite_or_raises(call):
    """True when ``call`` raises or returns a tensor (or list of tensors) with non-finite values; the value otherwise."""
    try:
        out = call()
    except Exception:
        return True, None
    return False, out


@pytest.mark.parametrize("precision", ["fp32", "f16x3", "f16mx2", "bf16", "fp8_mixed", "fp8"])
def test_tiled_sample_keeps_a_nan_condition_pixel_visible(precision):
    from tests.test_engine_gpu import build_sampler
    sampler = build_sampler(128)
    label = torch.tensor([0]).cuda()
    torch.manual_seed(5)
    raised, out = _nonfinite_or_raises(lambda: sampler.tiled_sample(batch_size=4, condition_x=_poison_pixel(_cond()).cuda(), class_label=label,
                                                                    num_sample_steps=2, precision=precision).cpu())
    assert raised or not torch.isfinite(out).all(), "a NaN pixel of the condition image gave a finite image"


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_untiled_sample_keeps_a_nan_condition_pixel_visible(precision):
    from tests.test_engine_gpu import build_sampler
    sampler = build_sampler(128)
    label = torch.tensor([0]).cuda()
    torch.manual_seed(5)
    raised, out = _nonfinite_or_raises(lambda: sampler.sample(batch_size=1, condition_x=_poison_pixel(_cond()).cuda(), class_label=label,
                                                              num_sample_steps=2, precision=precision).cpu())
    assert raised or not torch.isfinite(out).all(), "a NaN pixel of the condition image gave a finite image"


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_edm_tiled_sample_with_clamp_keeps_a_nan_condition_pixel_visible(precision):
    from tests.test_engine_gpu import build_edm_sampler
    sampler = build_edm_sampler(128)
    label = torch.tensor([0]).cuda()
    torch.manual_seed(5)
    raised, out = _nonfinite_or_raises(lambda: sampler.tiled_sample(batch_size=4, condition_x=_poison_pixel(_cond()).cuda(), class_label=label,
                                                                    num_sample_steps=2, clamp=True, precision=precision).cpu())
    assert raised or not torch.isfinite(out).all(), "a NaN pixel of the condition image gave a finite image"


@pytest.mark.parametrize("precision", ["fp32", "f16x3", "bf16"])
def test_lockstep_nan_stays_in_its_own_image(precision):
    # two images in lock-step, only the first poisoned: the second is bit-identical to its solo run (the project's claim for
    # lock-step), and the first is the one that comes out non-finite
    from tests.test_engine_gpu import build_sampler
    sampler = build_sampler(128)
    label = torch.tensor([0]).cuda()
    second = _cond(1)
    torch.manual_seed(5)
    solo = sampler.tiled_sample(batch_size=4, condition_x=second.cuda(), class_label=label, num_sample_steps=2, precision=precision).cpu()
    assert torch.isfinite(solo).all()
    conds = torch.cat([_poison_pixel(_cond(0)), second]).cuda()
    torch.manual_seed(5)
    raised, both = _nonfinite_or_raises(lambda: sampler.tiled_sample(batch_size=4, condition_x=conds, class_label=label, num_sample_steps=2,
                                                                     precision=precision).cpu())
    if raised:
        return
    assert not torch.isfinite(both[0]).all(), "a NaN pixel of the condition image gave a finite image"
    assert torch.equal(both[1:2], solo), "the poisoned image changed its lock-step neighbour"


@pytest.mark.parametrize("precision", ["f16x3", "bf16"])
def test_a_nan_weight_gives_a_nonfinite_image(precision):
    # how it happens in practice: no NaN in the inputs, one in a mid-network 3x3 convolution weight (a corrupt checkpoint, a
    # diverged fine-tune).  The NaN is born inside the U-Net and meets the sampler's x_start clamp first.
    import json
    import os
    from srgd_amd.synth import synth_state_dict
    from tests.test_engine_gpu import G, build_sampler
    with open(os.path.join(G, "schema_dim128.json")) as f:
        schema = {k: tuple(v) for k, v in json.load(f).items()}
    sd = synth_state_dict(schema, seed=0)
    key = "model.mid_block1.block1.proj.weight"
    assert sd[key].dim() == 4 and sd[key].shape[-1] == 3
    sd[key] = sd[key].clone()
    sd[key][17, 33, 1, 2] = float("nan")
    sampler = build_sampler(128, fresh=True)
    sampler.load_state_dict(sd, strict=True)
    sampler.model._invalidate_engines()
    label = torch.tensor([0]).cuda()
    torch.manual_seed(5)
    raised, out = _nonfinite_or_raises(lambda: sampler.tiled_sample(batch_size=4, condition_x=_cond().cuda(), class_label=label,
                                                                    num_sample_steps=2, precision=precision).cpu())
    del sampler
    assert raised or not torch.isfinite(out).all(), "a NaN weight gave a finite image"
