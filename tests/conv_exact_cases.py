"""Integer inputs for every convolution kernel path and epilogue, their exact outputs and GroupNorm sums, and the assertions
that go with them.

Pure torch on the CPU; test infrastructure only (used by tests/test_conv_exact_gpu.py, which feeds the tensors to the HIP kernels
through the kernel-level C ABI, and by tests/test_conv_exact_cases_cpu.py, which proves every condition below and shows that the
assertions reject a subtly wrong convolution).  Tensors are NCHW fp32 as tests/test_kernels_gpu.py's run_conv takes them.

Why integers: the random-data parity tests allow 1.2e-2 * max|ref| in bf16, about 0.05 where one product of a Cin >= 128 layer is
about 0.03 - a tap dropped, doubled or read from the wrong channel at one border or tile seam passes.  With small integers every
product and every partial sum is an exact integer below 2^24, so the result depends on no summation order, MFMA fragment layout or
tile shape: the kernel must equal the float64 convolution bit for bit (after `.to(bfloat16)` in bf16 mode).  Integers |v| <= 3 are
exact in bf16, in f16 (the `lo` halves of the split are zero, the power-of-two weight scale is exact) and in e4m3 under any
power-of-two block scale, so this holds in every reduced-precision kernel as well.
(The lo halves of the split, its cross products and the weight scale on non-integers: tests/split_exact_cases.py.)

The non-linear epilogues: the device SiLU is x / (1 + expf(-x)) or x * rcp(1 + __expf(-x)); for x >= 32, 1 + exp(-x) rounds to
exactly 1 in fp32, so SiLU is the identity on integers >= 32.  The reference below therefore APPLIES NO SiLU: the data make every
SiLU argument an integer >= SILU_MIN (Case.silu_args; the CPU file checks that fp32 F.silu is the identity on them):
  up       (SiLU + PixelShuffle)  bias = 32 + max|conv| + {0..4}
  tail     (ResnetBlock tail)     out = conv + silu(a*h + b): a in {1, 2, 3}, h in {-3..3}, b = 64
  staging  (GroupNorm-in-staging) conv(silu(a*x + b)): a in {1, 2}, x in {-1, 0, 1}, b = 34; the activated value is a non-zero
           integer, so a kernel that pads with silu(b) instead of zero fails at every border
Where something is added after the convolution (residual, tail) every value stays an integer <= 256 in magnitude: exact in bf16,
whichever of the additions a bf16 kernel rounds.

GroupNorm sums: where a case has groups, s2 = sum y^2 < 2^24 for every (sample, group) - then every partial sum of y and of y^2,
in any order and any slot partition, is an exact fp32 integer and the slot sums added in float64 must equal s1 and s2 exactly.  It
is enforced by thinning the weights to the density `stats_density`.
"""
import collections
import functools
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

SILU_MIN = 32                             # exp(-32) = 1.3e-14 < 2^-25: 1 + exp(-x) == 1 in fp32
EXACT_MAX = 2 ** 24                       # integers below it are exact in fp32
BF16_EXACT_MAX = 256                      # integers up to it are exact in bf16 (8 significant bits)
TAIL_B, STAGING_B = 64, 34


@dataclass(frozen=True)
class Spec:
    name: str
    layer: str                            # "3x3" (pad 1), "1x1", "down" (kind 1: 2x2 / stride 2 = unshuffle + 1x1), "up" (kind 2: 1x1 + SiLU + PixelShuffle)
    B: int
    C0: int
    C1: int
    Cout: int
    H: int
    W: int
    groups: int = 0                       # > 0: the GroupNorm partial sums are checked
    residual: bool = False
    tail: bool = False                    # out = conv + silu(a[b][o] * h + b[b][o])
    staging: bool = False                 # conv(silu(a[b][c] * x + b[b][c])), zero padding after the activation

    @property
    def taps(self):
        return {"3x3": 9, "1x1": 1, "down": 4, "up": 1}[self.layer]

    @property
    def K(self):                          # summed products per output element
        return self.taps * (self.C0 + self.C1)

    @property
    def small(self):                      # data in {-1, 0, 1}: keeps s2 < 2^24 / the sums of the additive epilogues exact in bf16
        return bool(self.groups or self.residual or self.tail or self.staging)

    def run_kw(self):
        """ks / stride / pad / kind of tests/test_kernels_gpu.py's run_conv."""
        return {"3x3": dict(ks=3, stride=1, pad=1, kind=0), "1x1": dict(ks=1, stride=1, pad=0, kind=0),
                "down": dict(ks=2, stride=2, pad=0, kind=1), "up": dict(ks=1, stride=1, pad=0, kind=2)}[self.layer]


@dataclass
class Case:
    spec: Spec
    x0: torch.Tensor
    x1: torch.Tensor                      # None: one source
    w: torch.Tensor                       # [Cout, taps' worth of input channels, k, k] as run_conv takes it
    bias: torch.Tensor
    residual: torch.Tensor                # None unless spec.residual
    tail: tuple                           # (h [B, Cout, H, W], a [B, Cout], b [B, Cout]) or None
    coef: tuple                           # staging: (a [B, C0], b [B, C0]) or None
    density: float
    want: torch.Tensor = None             # float64, the exact output
    s1: torch.Tensor = None               # float64 [B, groups]: sum of conv + bias per (sample, group); None without groups
    s2: torch.Tensor = None
    silu_args: torch.Tensor = None        # every value a SiLU of the kernel sees (None: no SiLU in this case)


def bf16_round(x):
    return x.to(torch.bfloat16).float()


def stats_density(spec):
    """E[y^2] = K * d * E[x^2] * E[w^2] + E[bias^2] = K * d * 4/9 + 2 for x, w uniform in {-1, 0, 1} (w kept with probability d)
    and bias uniform in {-2..2}; d puts cpg * H * W * E[y^2] at 0.6 * 2^24."""
    if not spec.groups:
        return 1.0
    n = (spec.Cout // spec.groups) * spec.H * spec.W // (4 if spec.layer == "down" else 1)
    return min(1.0, (0.6 * EXACT_MAX / n - 2) / (spec.K * 4 / 9))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _group_sums(pre, groups):
    b = pre.shape[0]
    return pre.reshape(b, groups, -1).sum(-1), (pre * pre).reshape(b, groups, -1).sum(-1)


def _not_mirrored(t, dims):
    return all(not torch.equal(t, t.flip(d)) for d in dims if t.shape[d] > 1)


Ref = collections.namedtuple("Ref", "out s1 s2 silu_args pre")      # pre: conv + bias, what the sums are taken of


def reference(c, mutant=None):
    """Ref in float64 from the case's inputs.  SiLU is taken as the identity (module docstring).
    `mutant`: one deliberate defect of those a kernel could have (MUTANTS); None is the reference itself."""
    s = c.spec
    x = (c.x0 if c.x1 is None else torch.cat((c.x0, c.x1), 1)).double()
    w, bias = c.w.double(), c.bias.double()
    args = []
    if mutant == "swap_seam":             # the last channel of source 0 and the first of source 1 read from each other's place
        idx = list(range(x.shape[1]))
        idx[s.C0 - 1], idx[s.C0] = idx[s.C0], idx[s.C0 - 1]
        x = x[:, idx]
    rows = list(range(s.B))
    if mutant == "swap_rows":             # the [b][c] coefficient rows of samples 0 and 1 exchanged
        rows[0], rows[1] = 1, 0
    pad = 1 if s.layer == "3x3" else 0
    if s.staging:
        a, b = c.coef[0].double()[rows, :, None, None], c.coef[1].double()[rows, :, None, None]
        x = a * x + b
        args.append(x)
        if mutant == "pad_silu_b":        # the halo filled before the activation: silu(a * 0 + b) = b instead of zero
            full = b.expand(-1, -1, s.H + 2, s.W + 2).clone()
            full[:, :, 1:-1, 1:-1] = x
            x, pad = full, 0
    if s.layer == "down":
        x = F.pixel_unshuffle(x, 2)       # 'b c (h p1) (w p2) -> b (c p1 p2) h w'
    pre = F.conv2d(x, w, bias, padding=pad)
    if mutant == "drop_tap":              # one product missing at the top-right output pixel of the last sample: its bottom-left tap
        k = w.shape[2]
        sy, sx = (k - 1) - pad, pre.shape[3] - 1 - pad
        ci = int(x[s.B - 1, :, sy, sx].nonzero()[0])
        pre = pre.clone()
        pre[s.B - 1, :, 0, -1] -= w[:, ci, k - 1, 0] * x[s.B - 1, ci, sy, sx]
    s1 = s2 = None
    if s.groups:
        s1, s2 = _group_sums(pre, s.groups)
        if mutant == "stats_skip":        # the bottom-left pixel of the last sample left out of the last group's sums
            y = pre[s.B - 1, -(s.Cout // s.groups):, -1, 0]
            s1, s2 = s1.clone(), s2.clone()
            s1[-1, -1] -= y.sum()
            s2[-1, -1] -= (y * y).sum()
    out = pre
    if s.layer == "up":
        args.append(pre)
        if mutant == "ps_transposed":     # channel c*4 + p1*2 + p2 lands at (2h + p2, 2w + p1)
            out = pre.reshape(s.B, s.Cout // 4, 2, 2, s.H, s.W).transpose(2, 3).reshape(pre.shape)
        out = F.pixel_shuffle(out, 2)
    if s.residual:
        out = out + c.residual.double()
    if s.tail:
        h, a, b = c.tail
        t = a.double()[rows, :, None, None] * h.double() + b.double()[rows, :, None, None]
        args.append(t)
        out = out + t
    return Ref(out, s1, s2, torch.cat([t.reshape(-1) for t in args]) if args else None, pre)


MUTANTS = ("drop_tap", "swap_seam", "stats_skip", "pad_silu_b", "ps_transposed", "swap_rows")


def mutant_applies(spec, mutant):
    return {"drop_tap": True, "swap_seam": spec.C1 > 0, "stats_skip": spec.groups > 0, "pad_silu_b": spec.staging,
            "ps_transposed": spec.layer == "up", "swap_rows": (spec.staging or spec.tail) and spec.B > 1}[mutant]


@functools.lru_cache(maxsize=None)
def build(spec):
    """The seeded inputs of a case and its exact output and sums.  Cached: the GPU file runs several kernels on one case; nobody
    may write to the tensors.  Asserts the conditions the exactness argument rests on (they are conditions, not measurements)."""
    g = torch.Generator().manual_seed(5 + zlib.crc32(spec.name.encode()) % 10007)
    s = spec
    amp_x, amp_w = (1, 1) if s.small else (3, 2)
    x0 = _randint(g, -amp_x, amp_x, (s.B, s.C0, s.H, s.W))
    x1 = _randint(g, -amp_x, amp_x, (s.B, s.C1, s.H, s.W)) if s.C1 else None
    k = 3 if s.layer == "3x3" else 1
    cin = (s.C0 + s.C1) * (4 if s.layer == "down" else 1)
    w = _randint(g, -amp_w, amp_w, (s.Cout, cin, k, k))
    d = stats_density(s)
    if d < 1.0:
        w = w * (torch.rand(w.shape, generator=g) < d)
    bias = _randint(g, -2, 2, (s.Cout,)) if s.small else _randint(g, -4, 4, (s.Cout,))
    c = Case(s, x0, x1, w, bias, None, None, None, d)
    if s.staging:
        c.coef = (_randint(g, 1, 2, (s.B, s.C0)), torch.full((s.B, s.C0), float(STAGING_B)))
    if s.layer == "up":
        conv = reference(Case(s, x0, x1, w, torch.zeros(s.Cout), None, None, None, d)).pre
        c.bias = SILU_MIN + float(conv.abs().max()) + _randint(g, 0, 4, (s.Cout,))
    if s.residual:
        c.residual = _randint(g, -3, 3, (s.B, s.Cout, s.H, s.W))
    if s.tail:
        c.tail = (_randint(g, -3, 3, (s.B, s.Cout, s.H, s.W)), _randint(g, 1, 3, (s.B, s.Cout)), torch.full((s.B, s.Cout), float(TAIL_B)))
    ref = reference(c)
    c.want, c.s1, c.s2, c.silu_args = ref.out, ref.s1, ref.s2, ref.silu_args
    # ---- the conditions
    assert (w != 0).any(0).all(), f"{s.name}: a (tap, input channel) without a non-zero weight at density {d:.2f}"
    assert float(c.want.abs().max()) < EXACT_MAX and torch.equal(c.want, c.want.round())
    if s.groups:
        assert float(c.s2.max()) < EXACT_MAX, f"{s.name}: max s2 = {float(c.s2.max()) / EXACT_MAX:.2f} * 2^24"
    if c.silu_args is not None:
        assert float(c.silu_args.min()) >= SILU_MIN, f"{s.name}: a SiLU argument of {float(c.silu_args.min())}"
    if s.residual or s.tail:
        assert float(c.want.abs().max()) <= BF16_EXACT_MAX and float(ref.pre.abs().max()) <= BF16_EXACT_MAX, s.name
    # no draw symmetric under a flip in y, x or channel order (a mirrored tap / channel index must show)
    assert _not_mirrored(x0, (1, 2, 3)) and _not_mirrored(w, (0, 1, 2, 3)) and _not_mirrored(c.bias, (0,)), s.name
    assert x1 is None or _not_mirrored(x1, (1, 2, 3))
    for t in (c.coef, c.tail[1:] if c.tail else None):
        assert t is None or s.B == 1 or not torch.equal(t[0][0], t[0][1]), f"{s.name}: equal coefficient rows"
    return c


# ---------------------------------------------------------------------------------------------- the assertions both files use
def expected(case, bf16):
    want = case.want.float()
    return bf16_round(want) if bf16 else want


def assert_output(case, got, bf16):
    """`got`: the kernel's output as fp32 NCHW on the CPU."""
    want = expected(case, bf16)
    assert got.shape == want.shape, (case.spec.name, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        first = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError("%s: %d of %d elements differ from the exact value; first at [b, c, y, x] = %s: got %r, want %r" % (
            case.spec.name, int(bad.sum()), bad.numel(), first, float(got[tuple(first)]), float(want[tuple(first)])))


def assert_sums(case, sums):
    """`sums`: float64 [B, groups, 2], the partial slots added on the host."""
    want = torch.stack((case.s1, case.s2), -1)
    assert sums.dtype == torch.float64 and sums.shape == want.shape, (case.spec.name, sums.dtype, tuple(sums.shape))
    if not torch.equal(sums, want):
        bad = ((sums != want) | torch.isnan(sums)).any(-1)
        b, grp = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError("%s: the GroupNorm sums of %d of %d (sample, group) pairs differ; first at (b, group) = (%d, %d): got "
                             "(s1, s2) = %s, want %s" % (case.spec.name, int(bad.sum()), bad.numel(), b, grp, sums[b, grp].tolist(),
                                                         want[b, grp].tolist()))


def assert_equal_tensors(name, a, b, what):
    """Two kernels on one case: a consequence of exactness, kept as its own assertion for the next refactor."""
    if not torch.equal(a, b):
        bad = (a != b) | torch.isnan(a) | torch.isnan(b)
        first = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError("%s: %s differ in %d of %d elements; first at %s: %r vs %r" % (
            name, what, int(bad.sum()), bad.numel(), first, float(a[tuple(first)]), float(b[tuple(first)])))


def slot_capacity(spec):
    """include/srgd_hip_kernels.h: nslots_capacity = (Hout * Wout / 32) * max(1, (Cout / groups) / 64)."""
    hw = spec.H * spec.W // (4 if spec.layer == "down" else 1)
    return (hw // 32) * max(1, spec.Cout // spec.groups // 64)


# ---------------------------------------------------------------------------------------------- the table
# The smallest shapes that still reach every code path; nothing is at the workload's size.  (B, C0, C1, Cout, H, W[, groups]).
def _s(name, layer, shape, **kw):
    return Spec(name, layer, *shape[:6], groups=shape[6] if len(shape) > 6 else 0, **kw)


# Halo-patch 3x3 kernels (8 x 32 pixel patches, 128-channel n-tiles), each channels-per-group class of the register-direct epilogue
HALO = [
    _s("halo_cpg16_one_patch", "3x3", (2, 32, 0, 128, 8, 32, 8)),             # one patch per image: both borders in every patch
    _s("halo_cpg32_two_sources", "3x3", (1, 64, 32, 256, 16, 64, 8)),         # 2 n-tiles, interior seams
    _s("halo_cpg16_B3", "3x3", (3, 128, 0, 128, 32, 32, 8)),
    _s("halo_cpg128", "3x3", (1, 256, 128, 1024, 8, 32, 8)),
    _s("halo_cpg64", "3x3", (2, 32, 0, 512, 16, 32, 8)),                      # one group per wave
    _s("halo_cpg256", "3x3", (1, 32, 0, 2048, 16, 32, 8)),                    # a group spans two tiles
    _s("halo_no_stats", "3x3", (1, 32, 0, 2048, 8, 32, 0)),
]
HALO_IMPLS = [(2, True), (6, False), (8, False), (12, False), (14, False)]    # (impl, bf16 tensors)

# the same kernels with GroupNorm-in-staging (one source: the rule of impl 5 / 11 / 13 / 15).  Output only; the outputs are in the
# thousands, so the bf16 output rounding is exercised
STAGING = [
    _s("staging_B2", "3x3", (2, 64, 0, 128, 16, 32), staging=True),
    _s("staging_B3", "3x3", (3, 32, 0, 128, 8, 32), staging=True),
]
STAGING_IMPLS = [(5, True), (11, False), (13, False), (15, False)]

# srgd_k_conv3x3_mxfp8 (its own entry point; C0, C1, Cout % 128 == 0)
MX3 = [
    _s("mx3_cpg16_B2", "3x3", (2, 128, 0, 128, 8, 32, 8)),
    _s("mx3_cpg32_two_sources", "3x3", (1, 128, 256, 256, 16, 64, 8)),
    _s("mx3_cpg64", "3x3", (1, 128, 0, 512, 8, 32, 8)),
    _s("mx3_cpg128", "3x3", (1, 128, 0, 1024, 8, 32, 8)),
    _s("mx3_cpg256", "3x3", (1, 128, 0, 2048, 8, 32, 8)),
]

# Generic implicit GEMM (128 x 128 tiles): impl 1 in fp32 and bf16, impl 7 / 9 (split operands, f16 / bf16 halves; Cout is padded to
# the n-tile inside the call, so the ragged case keeps Cout = 40)
GENERIC = [
    _s("generic_3x3_stats", "3x3", (2, 32, 0, 64, 16, 16, 8)),
    _s("generic_3x3_stats_6_groups", "3x3", (3, 32, 0, 96, 16, 8, 6)),
    _s("generic_3x3_two_sources_residual", "3x3", (2, 64, 32, 48, 16, 32), residual=True),
    _s("generic_3x3_ragged_m", "3x3", (3, 32, 0, 40, 10, 10)),                 # 100 pixels per sample: a masked 128-row tile
    _s("generic_1x1_two_sources", "1x1", (2, 64, 32, 160, 16, 32)),
    _s("generic_unshuffle", "down", (2, 32, 0, 64, 32, 32)),
    _s("generic_pixel_shuffle", "up", (2, 64, 0, 128, 16, 16)),
]
GENERIC_IMPLS = [(1, False), (1, True), (7, False), (9, False)]

# Streaming pointwise kernels: B = 3, 16 x 32 outputs = two 256-pixel tiles per image
STREAM = [
    _s("stream_plain", "1x1", (3, 64, 32, 256, 16, 32)),
    _s("stream_residual", "1x1", (3, 64, 32, 256, 16, 32), residual=True),
    _s("stream_gn_tail", "1x1", (3, 64, 32, 256, 16, 32), tail=True),
    _s("stream_pixel_shuffle", "up", (3, 64, 0, 1024, 16, 32)),               # Cout / 4 = 256: two n-tiles per sub-pixel
    _s("stream_unshuffle", "down", (3, 32, 0, 128, 32, 64)),
    _s("stream_k_heavy", "1x1", (3, 512, 256, 128, 16, 32)),
]
STREAM_IMPLS = [(3, True), (10, False)]


def _to_128(spec):
    """impl 4 (conv1x1_mxfp8: C0, C1, Cout % 128 == 0): the same case with every channel count raised to a multiple of 128."""
    up = lambda n: -(-n // 128) * 128
    return Spec(spec.name.replace("stream_", "stream_mx_"), spec.layer, spec.B, up(spec.C0), up(spec.C1), up(spec.Cout), spec.H, spec.W,
                residual=spec.residual, tail=spec.tail)


STREAM_MX = [_to_128(s) for s in STREAM]

# family -> (cases, tensor types the family runs in, whether a split-operand (f16) / MX kernel takes the case)
FAMILIES = {
    "halo": (HALO, ("bf16", "fp32")), "staging": (STAGING, ("bf16", "fp32")), "mx3": (MX3, ("bf16",)),
    "generic": (GENERIC, ("bf16", "fp32")), "stream": (STREAM, ("bf16", "fp32")), "stream_mx": (STREAM_MX, ("bf16",)),
}
ALL = [s for cases, _ in FAMILIES.values() for s in cases]
assert len({s.name for s in ALL}) == len(ALL)


def family_of(spec):
    return next(f for f, (cases, _) in FAMILIES.items() if spec in cases)
