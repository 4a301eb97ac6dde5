"""GroupNorm at large group means: inputs that put a group's mean many standard deviations from zero, float64 and fp32 references of
the Block tail on a given convolution output, an emulation of the sum / sum-of-squares statistics, and the gates that go with them.

Pure torch on the CPU; test infrastructure only (used by tests/test_groupnorm_conditioning_gpu.py, which feeds the tensors to the HIP
kernels and the engine, and by tests/test_groupnorm_cases_cpu.py, which shows that the reference's own fp32 arithmetic stays inside
every gate and that the gates reject the emulated scheme where its error model says they must).  Tensors are NCHW fp32 as
tests/test_kernels_gpu.py's run_conv takes them.

Why: every statistics producer writes fp32 partial sums of y and y^2; var = s2/n - mean^2 then loses about mean^2 / var * 2^-24 of
its relative accuracy, whatever the precision of the final additions.  The synthetic weights of every other fixture have biases
of 0.02 * randn and zero-mean kernels, so every group mean there is about 0 and the loss never shows.  A trained network's groups
are bias-dominated as a matter of course.  The ratio R = |mean| / std of a group is the knob:

  bias-borne   x ~ N(0, 1), zero-mean weights scaled for an output std of SIGMA, bias = (+-R * SIGMA per group) + 0.02 * randn
  data-borne   x = DC + randn / 16, bias = 0.02 * randn; the weights of the eight outer taps sum to zero over the input channels
               (the DC passes through none of them, so the zero padding leaves no border step), the centre tap carries
               +-R * SIGMA / (Cin * DC) per input channel on top: the group mean arrives through the accumulation, no bias pivot
               can remove it

The kernel cases are the smallest shapes of the existing tests that reach every statistics producer and every branch of the halo
kernels' partial-sum store (16, 32, 64 and 128 channels per group).  The engine cases shift every `*.proj.bias` (the convolution
in front of each GroupNorm) by a per-group constant drawn uniformly in +-M.
"""
import functools
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

RATIOS = (0, 8, 64, 512)
MODES = ("bias", "data")
SIGMA = 1.0                               # standard deviation of the convolution output around its group mean
DC = 32.0                                 # data-borne: the input's offset (its noise is 1 / 16: the offset is 512 of them)
SLOT_PIXELS = 64                          # pixels per partial-sum slot of the emulation (one wave's share of a 256-pixel patch)
EPS = 1e-5


# ---------------------------------------------------------------------------------------------- kernel cases
@dataclass(frozen=True)
class Spec:
    shape: str
    B: int
    C0: int
    C1: int
    Cout: int
    H: int
    W: int
    groups: int
    ratio: int
    mode: str

    @property
    def name(self):
        return "%s-R%d-%s" % (self.shape, self.ratio, self.mode)

    @property
    def cpg(self):
        return self.Cout // self.groups


@dataclass
class Case:
    spec: Spec
    x0: torch.Tensor
    x1: torch.Tensor                      # None: one source
    w: torch.Tensor
    bias: torch.Tensor
    gamma: torch.Tensor
    beta: torch.Tensor
    ss: torch.Tensor                      # [B, 2 * Cout]: scale | shift
    res: torch.Tensor


# (B, C0, C1, Cout, H, W, groups)
GENERIC_SHAPES = {"generic_g8": (2, 32, 0, 64, 16, 16, 8), "generic_g6": (3, 32, 0, 96, 16, 8, 6)}
HALO_SHAPES = {"halo_cpg16": (2, 32, 0, 128, 8, 32, 8), "halo_cpg32_two_sources": (1, 64, 32, 256, 16, 64, 8),
               "halo_cpg64": (3, 128, 0, 128, 32, 32, 2), "halo_cpg128": (3, 128, 0, 128, 32, 32, 1)}
SHAPES = dict(GENERIC_SHAPES, **HALO_SHAPES)

# producer -> (impl of run_conv or None for srgd_k_conv3x3_mxfp8, bf16 tensors, shapes)
_MX_SHAPES = [k for k, s in HALO_SHAPES.items() if s[1] % 128 == 0 and s[2] % 128 == 0 and s[3] % 128 == 0]   # the MX-fp8 kernel's rule
PRODUCERS = {
    "generic_fp32": (1, False, list(GENERIC_SHAPES)),
    "generic_bf16": (1, True, list(GENERIC_SHAPES)),
    "conv3x3_bf16": (2, True, list(HALO_SHAPES)),
    "conv3x3_split_512": (6, False, list(HALO_SHAPES)),
    "conv3x3_split_256": (12, False, list(HALO_SHAPES)),
    "conv_igemm_split": (7, False, list(HALO_SHAPES)),
    "conv3x3_mx2": (14, False, list(HALO_SHAPES)),
    "conv3x3_mxfp8": (None, True, _MX_SHAPES),
}
BF16_GATED_RATIOS = (0, 8)                # beyond: bf16's quantum (2^-8 of the mean) exceeds the group's spread


def spec(shape, ratio, mode):
    return Spec(shape, *SHAPES[shape], ratio=ratio, mode=mode)


ALL = [spec(s, r, m) for s in SHAPES for r in RATIOS for m in MODES]


def bf16_round(x):
    return x.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def build(s, bf16=False):
    """The case's tensors; `bf16`: activations and weights rounded to bf16 as the bf16 kernels' tests do.  Cached: read only."""
    g = torch.Generator().manual_seed(zlib.crc32(s.name.encode()))
    cin = s.C0 + s.C1
    sign = torch.where(torch.rand(s.groups, generator=g) < 0.5, -1.0, 1.0)
    if s.groups > 1:
        sign[0], sign[1] = 1.0, -1.0                                         # both signs in every case
    level = (sign * s.ratio * SIGMA).repeat_interleave(s.cpg)               # [Cout]: the group means
    w = torch.randn(s.Cout, cin, 3, 3, generator=g)
    jitter = 0.02 * torch.randn(s.Cout, generator=g)
    if s.mode == "bias":
        x = torch.randn(s.B, cin, s.H, s.W, generator=g)
        w = w * (SIGMA / (3 * cin ** 0.5))
        bias = level + jitter
    else:
        noise = 1.0 / 16
        x = DC + noise * torch.randn(s.B, cin, s.H, s.W, generator=g)
        w = w - w.mean(1, keepdim=True)                                      # every tap sums to zero over the input channels
        w = w * (SIGMA / (3 * cin ** 0.5 * noise))
        w[:, :, 1, 1] += (level / (cin * DC))[:, None]
        bias = jitter
    gamma, beta = 1 + 0.2 * torch.randn(s.Cout, generator=g), 0.3 * torch.randn(s.Cout, generator=g)
    ss = 0.5 * torch.randn(s.B, 2 * s.Cout, generator=g)
    res = torch.randn(s.B, s.Cout, s.H, s.W, generator=g)
    if bf16:
        x, w, res = bf16_round(x), bf16_round(w), bf16_round(res)
    x0, x1 = (x, None) if not s.C1 else (x[:, :s.C0].contiguous(), x[:, s.C0:].contiguous())
    return Case(s, x0, x1, w, bias, gamma, beta, ss, res)


def conv_output(c, dtype=torch.float32):
    """The convolution the producers compute, on the CPU (the GPU tests take the device's own output instead)."""
    x = c.x0 if c.x1 is None else torch.cat((c.x0, c.x1), 1)
    return F.conv2d(x.to(dtype), c.w.to(dtype), c.bias.to(dtype), padding=1)


def measured_ratio(y, groups):
    """min and max over (sample, group) of |mean| / std of a convolution output."""
    v = y.double().reshape(y.shape[0], groups, -1)
    r = v.mean(-1).abs() / v.std(-1, unbiased=False)
    return float(r.min()), float(r.max())


# ---------------------------------------------------------------------------------------------- references
def _tail(yn, ss, res):
    if ss is not None:
        cout = yn.shape[1]
        yn = yn * (ss[:, :cout, None, None].to(yn.dtype) + 1) + ss[:, cout:, None, None].to(yn.dtype)
    out = F.silu(yn)
    return out if res is None else out + res.to(yn.dtype)


def reference(y, groups, gamma, beta, ss=None, res=None, dtype=torch.float64):
    """silu(gn(y) * (scale + 1) + shift) + res (reference Block.forward + the ResnetBlock residual) in `dtype`: float64 is the
    expectation, float32 the reference's own arithmetic (torch's group_norm, as the reference runs it)."""
    yn = F.group_norm(y.to(dtype), groups, gamma.to(dtype), beta.to(dtype), eps=EPS)
    return _tail(yn, ss, res)


def sum_of_squares_mutant(y, groups, gamma, beta, ss=None, res=None):
    """The scheme under test, emulated: fp32 sums of y and y^2 over slots of SLOT_PIXELS pixels x the group's channels, the slots
    added in float64, var = s2/n - mean^2, then the finalize / apply arithmetic in fp32 (y * A + B with A = rstd * gamma,
    B = beta - mean * A, the scale and shift folded in)."""
    b, c, h, w = y.shape
    cpg, hw = c // groups, h * w
    assert hw % SLOT_PIXELS == 0
    v = y.float().reshape(b, groups, cpg, hw // SLOT_PIXELS, SLOT_PIXELS).permute(0, 1, 3, 2, 4).reshape(b, groups, hw // SLOT_PIXELS, -1)
    s1 = v.sum(-1).double().sum(-1)
    s2 = (v * v).sum(-1).double().sum(-1)
    n = float(cpg * hw)
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0.0)
    rstd = (1.0 / (var + EPS).sqrt()).float().repeat_interleave(cpg, 1)     # [B, C]
    fmean = mean.float().repeat_interleave(cpg, 1)
    a = rstd * gamma.float()
    bb = beta.float() - fmean * a
    if ss is not None:
        sc, sh = ss[:, :c].float() + 1.0, ss[:, c:].float()
        a, bb = a * sc, bb * sc + sh
    out = F.silu(a[:, :, None, None] * y.float() + bb[:, :, None, None])
    return out if res is None else out + res.float()


def err(got, want64):
    return float((got.double() - want64).abs().max())


# ---------------------------------------------------------------------------------------------- gates
def floor(bf16, want, k=2.0):
    """tests/test_kernels_gpu.py's `tol(bf16, want, k=2.0)`: what test_conv_groupnorm_scale_shift_silu_residual allows."""
    return (1.2e-2 if bf16 else 2e-5) * max(1.0, float(want.abs().max())) * k


def kernel_gate(e_ref, want):
    """fp32 tensors: four times the reference's own fp32 rounding on the same values (room for another sound summation order,
    none for the 10x - 100x of the sum-of-squares scheme), or the floor the well-conditioned case meets."""
    return max(4.0 * e_ref, floor(False, want))


def engine_gate(e_ref, want):
    """Whole forward: four times the fp32 oracle's own distance from float64, or test_unet_forward_matches_reference's 1e-4 * scale."""
    return max(4.0 * e_ref, 1e-4 * max(1.0, float(want.abs().max())))


# ---------------------------------------------------------------------------------------------- engine cases
ENGINE_MS = (8, 32, 128)
ENGINE_DIMS = (16, 128)
ENGINE_HW = 64


def shifted_state_dict(schema, seed, M, groups=8):
    """srgd_amd.synth weights with every `*.proj.bias` (the convolution in front of a GroupNorm) moved by a per-group constant drawn
    uniformly in +-M: the draw depends on the key alone, M scales it.  fp32, as the engine loads it - the float64 expectation is
    taken on `.double()` of THIS dict, after bias + offset has been rounded per channel."""
    from srgd_amd.synth import synth_state_dict
    sd = synth_state_dict(schema, seed=seed)
    if not M:
        return sd
    for k in sorted(sd):
        if k.endswith(".proj.bias"):
            g = torch.Generator().manual_seed(zlib.crc32(k.encode()) + 7919)
            u = torch.rand(groups, generator=g) * 2 - 1
            sd[k] = sd[k] + (float(M) * u).repeat_interleave(sd[k].numel() // groups)
    return sd


def engine_inputs(dim, batch=1):
    g = torch.Generator().manual_seed(900 + dim)
    x = torch.randn(batch, 3, ENGINE_HW, ENGINE_HW, generator=g)
    cnd = torch.rand(batch, 3, ENGINE_HW, ENGINE_HW, generator=g) * 2 - 1
    ls = torch.tensor([0.75, -1.5, 2.0][:batch], dtype=torch.float32)
    return x, cnd, ls, torch.tensor([1])


def oracle_forward(sd, dim, x, cnd, ls, label, dtype, group_norm=None):
    """oracle.srgd_oracle.unet_forward on `sd` in `dtype`; `group_norm`: a stand-in for F.group_norm inside it (the mutant)."""
    from oracle import srgd_oracle as O
    usd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in O.strip_model_prefix(sd).items()}
    keep = F.group_norm
    try:
        if group_norm is not None:
            F.group_norm = group_norm
        with torch.inference_mode():
            return O.unet_forward(usd, O.UnetCfg(dim=dim), x.to(dtype), ls.to(dtype), label, cnd.to(dtype))
    finally:
        F.group_norm = keep


def mutant_group_norm(x, groups, weight, bias, eps=EPS):
    """F.group_norm's signature on the emulated scheme (slots of SLOT_PIXELS pixels; fewer when the image has fewer)."""
    b, c, h, w = x.shape
    cpg, hw = c // groups, h * w
    sp = min(SLOT_PIXELS, hw)
    v = x.reshape(b, groups, cpg, hw // sp, sp).permute(0, 1, 3, 2, 4).reshape(b, groups, hw // sp, -1)
    s1, s2 = v.sum(-1).double().sum(-1), (v * v).sum(-1).double().sum(-1)
    n = float(cpg * hw)
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0.0)
    a = (1.0 / (var + eps).sqrt()).float().repeat_interleave(cpg, 1) * weight
    bb = bias - mean.float().repeat_interleave(cpg, 1) * a
    return a[:, :, None, None] * x + bb[:, :, None, None]
