"""Closed-form cases for srgd_amd/csrc/norm_act.hip: ``gn_apply_kernel`` without the MX-fp8 twin (every instance: fp32 PRECISE with
HOIST on and off, bf16 with HOIST on and off) and ``rms_norm_kernel`` (fp32, bf16).  CPU only: constructions, float64 references,
tolerances derived from the oracle alone, launch models restated from the source comments, and mutants.
tests/test_norm_cases_cpu.py proves the constructions and shows that every assertion rejects every mutant;
tests/test_norm_exact_gpu.py feeds the cases to the kernels.

Two exactness devices (fp32; asserted on the CPU by ``assert_silu_device``):
  * SiLU is the identity or zero: for t >= 32, 1 + exp(-t) is exactly 1, so t / (1 + exp(-t)) = t; for t <= -96, exp(-t) = +inf and
    t / inf = -0.  Both hold for the expf form and for the __expf + rcp form (rcp(1) = 1, rcp(inf) = 0).
  * With small-integer coefficients, inputs and residuals every value is an integer below 2^24 (bf16 tensors: below 256, an exact
    bf16), the same in any summation order, with or without FMA contraction - compared BIT FOR BIT, -0 == +0.

RMSNorm's exact rows: C = 2^n channels, a row has m = C / 4^i non-zero entries +-a with a a power of two, so ss = m a^2,
sqrtf(ss) and sqrtf(C) / sqrtf(ss) = 2^i / a are exact (for odd n both roots carry the same rounded sqrt 2 and the correctly
rounded quotient is exact again); the gains are dyadic with 8 significant bits; the output is +-g_c 2^i bit for bit.

Not tested: |x| so large that the sum of squares overflows - the reference (F.normalize in fp32) overflows there too.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from oracle import srgd_oracle as O

MARGIN = 8                      # the project's convention: MARGIN x (the oracle's own fp32 evaluation against float64) ...
FLOOR_ULPS = 4                  # ... with a floor of 4 ulp of the tensor's largest magnitude
MUTANT_FACTOR = 100
BF16_SUB = 2.0 ** -134          # half a step of bf16's subnormals
SILU_ID_MIN, SILU_ZERO_MAX = 32, -96
PERIOD = 1021                   # prime: no sample, block or grid-stride boundary lines up with the data
GUARD = 64                      # elements of guard band on either side of an output
EPS_NORM = float(np.float32(1e-12))


def ulp32(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(v)) - 23) if v > 0 else 2.0 ** -149


def distance(a, b) -> float:
    """max |a - b| in float64; NaN in the same places counts as equal, anything else non-finite as infinite."""
    a, b = a.double(), b.double()
    both_nan = torch.isnan(a) & torch.isnan(b)
    d = torch.where(both_nan, torch.zeros_like(a), (a - b).abs())
    return float("inf") if not bool(torch.isfinite(d).all()) else float(d.max()) if d.numel() else 0.0


def exact_factor(mutant, want) -> float:
    """An exact assertion admits no error at all; the factor of a mutant against it is its largest error in fp32 ulps of the
    largest expected magnitude (the coarsest ulp of the tensor: a lower bound of the error in the element's own ulps)."""
    return distance(mutant, want) / ulp32(float(want.abs().max()))


def rows_of(base: torch.Tensor, first: int, count: int) -> torch.Tensor:
    """Rows first .. first + count of the tensor whose row r is base[r % len(base)]."""
    return base[(torch.arange(first, first + count) % base.shape[0])]


def _hash(*idx):
    h = torch.zeros((), dtype=torch.int64)
    for k, v in zip((7919, 104729, 1299709), idx):
        h = h + v.to(torch.int64) * k
    h = (h * 2654435761) & 0xFFFFFFFF
    return (h ^ (h >> 15)) & 0x7FFFFFFF


def bf16_store_bound(ref: torch.Tensor) -> torch.Tensor:
    """The storage rounding of a bf16 tensor: half a bf16 step at the bf16 rounding of the REFERENCE (never at the result under test:
    a wrong result in a higher binade must not widen its own bound) - 8 significant bits, so 2^(e - 8) for a value in
    [2^e, 2^(e + 1)): 2^-9 of the value at the top of a binade, 2^-8 at its bottom.  (2^-9 of the value everywhere cannot hold:
    silu(0.015564) = 0.00784254 lies 3.0e-5 = 0.98 half-steps above the bf16 value 2^-7 it correctly rounds to, 2^-8.03 of it.)
    A reference that rounds UP to a power of two is granted the half step of the binade above, twice what its own binade has: the
    correct store then sits in that binade."""
    stored = ref.float().to(torch.bfloat16).double()
    e = torch.floor(torch.log2(stored.abs().clamp_min(2.0 ** -126)))
    return (2.0 ** (e - 8)).clamp_min(BF16_SUB)


def assert_silu_device():
    """The first exactness device, in fp32 on the CPU, in both forms the kernels use."""
    t = torch.tensor([32.0, 33.0, 40.0, 196.0, 1e4, 2.0 ** 23 + 1], dtype=torch.float32)
    z = torch.tensor([-96.0, -97.0, -104.0, -452.0, -1e4], dtype=torch.float32)
    for form in (lambda v: v / (1 + torch.exp(-v)), lambda v: v * (1 / (1 + torch.exp2(-v * 1.4426950408889634)))):
        assert torch.equal(form(t), t)
        assert torch.equal(form(z), torch.zeros_like(z)) and bool(torch.signbit(form(z)).all())


# ------------------------------------------------------------------------------------------------ 1. gn_apply: the launch model
@dataclass(frozen=True)
class GnLaunch:
    B: int
    vpp: int              # 16-byte vectors per pixel
    pow2: bool
    hoist: bool           # coefficients loaded once per thread
    n: int                # vectors per sample
    gx: int
    stride: int           # grid stride in vectors
    trips: frozenset      # {(four-vector trips, single trips)} over the threads that do any work


def gn_launch(B, hw, C, bf16) -> GnLaunch:
    """The launch gn_apply_silu (norm_act.hip) makes, restated from its comments: 16-byte vectors (N = 4 fp32, 8 bf16), one grid
    row per sample, "~64 blocks per CU over the whole launch, at least one block per sample" of 256 threads:
    gx = max(1, min(ceil(vps / 256), ceil(256 * 64 / B))); HOIST "when the grid stride is a multiple of the vectors per pixel
    (C / N a power of two <= 256)"; pow2: the channel offset is a mask instead of a remainder.  A thread starting at i0 < n walks
    i0, i0 + stride, ...: ceil((n - i0) / stride) vectors, four per trip while four remain, then one by one."""
    N = 8 if bf16 else 4
    assert C % N == 0
    vpp, n = C // N, hw * C // N
    gx = max(1, min((n + 255) // 256, (256 * 64 + B - 1) // B))
    stride = gx * 256
    pow2 = vpp & (vpp - 1) == 0
    most = -(-n // stride)
    counts = {most} | ({most - 1} if (n - 1) % stride + 1 < min(n, stride) else set())
    return GnLaunch(B, vpp, pow2, pow2 and vpp <= 256, n, gx, stride, frozenset((k // 4, k % 4) for k in counts if k > 0))


@dataclass(frozen=True)
class GnShape:
    B: int
    hw: int
    C: int
    groups: int
    bf16: bool
    in_place: bool
    residual: bool

    @property
    def id(self):
        return "%s_B%d_hw%d_C%d%s%s" % ("bf16" if self.bf16 else "fp32", self.B, self.hw, self.C, "_inplace" if self.in_place else "",
                                        "_res" if self.residual else "")

    @property
    def large(self):
        return self.B * self.hw * self.C > (1 << 24)


# B = 1, 2 and 4096; HOIST (C / N = 4, 16, 32); !HOIST with C / N no power of two (C = 96: 24 and 12); !HOIST with a power of two
# above 256 (C = 2048 fp32: 512); several blocks per sample with a ragged last block (hw = 131, 67); B = 4096 (gx = 4, stride 1024)
# with 4 * 1031 = 4124 and 4 * 1543 = 6172 vectors per sample: threads with 4 | 5 and 6 | 7 vectors, i.e. one four-vector trip and
# 0, 1, 2, 3 single trips.  Those two are the smallest launches that reach them (270 MB fp32, 404 MB bf16): a thread has four
# vectors only when the tensor holds more than 3 * 256 * 64 * 256 of them, whatever B.
GN_SHAPES = (
    GnShape(1, 67, 16, 8, False, False, False),
    GnShape(2, 131, 128, 8, False, False, True),
    GnShape(2, 67, 96, 6, False, True, True),
    GnShape(1, 5, 2048, 8, False, True, False),
    GnShape(4096, 1031, 16, 8, False, True, True),
    GnShape(1, 67, 32, 8, True, True, False),
    GnShape(2, 131, 128, 8, True, False, True),
    GnShape(2, 67, 96, 6, True, False, False),
    GnShape(2, 67, 96, 6, True, True, True),
    GnShape(4096, 1543, 32, 8, True, False, True),
)
COEF_PERIOD = 18                 # the coefficients of sample b are those of sample b % 18 (lcm of the periods below)


def unit_stats(hw, cpg):
    """(sum, sum of squares) of one statistics slot for which gn_finalize gives mean = 0 and rstd = 1.0f exactly:
    rstd = float(1 / sqrt(s2 / n + eps)) is 1.0f for s2 / n + eps in (1 - 2^-23, 1 + 2^-24); an fp32 s2 next to n (1 - eps) lands
    within 2^-24 of the centre of that window.  Returns the candidate closest to it; the CPU test asserts the float64 restatement."""
    n = float(hw * cpg)
    eps = float(np.float32(1e-5))
    centre = 1.0 - 2.0 ** -25
    s2 = np.float32(n * (centre - eps))
    cands = [np.nextafter(s2, np.float32(0)), s2, np.nextafter(s2, np.float32(np.inf))]
    best = min(cands, key=lambda c: abs(float(c) / n + eps - centre))
    return 0.0, float(best)


def finalize64(s1, s2, hw, cpg):
    """gn_finalize's statistics, restated: float64 mean and variance of one slot, rstd rounded to fp32."""
    n = float(hw * cpg)
    mean = s1 / n
    var = max(s2 / n - mean * mean, 0.0)
    return float(np.float32(mean)), float(np.float32(1.0 / math.sqrt(var + float(np.float32(1e-5)))))


@dataclass
class GnCase:
    shape: GnShape
    base_x: torch.Tensor           # fp32 [PERIOD, C] integers: pixel r = b * hw + p of the tensor is base_x[r % PERIOD]
    base_res: torch.Tensor         # fp32 [PERIOD, C] integers or None
    gamma: torch.Tensor            # fp32 [C]
    beta: torch.Tensor
    scale_shift: torch.Tensor      # fp32 [B, 2C]
    partial: torch.Tensor          # fp32 [B, groups, 1, 2]
    A: torch.Tensor                # float64 [COEF_PERIOD, C]: what gn_finalize must hand to gn_apply for sample b % COEF_PERIOD
    Bc: torch.Tensor
    want_table: torch.Tensor       # fp32 [COEF_PERIOD, PERIOD, C]: expected output of pixel r of sample b at [b % COEF_PERIOD, r % PERIOD]


def gn_coefs(C, B):
    """gamma in {1, 2}, beta in -2..2, scale in {0, 1} (so scale + 1 in {1, 2}), shift in -4..4: A = gamma (scale + 1) in {1, 2, 4},
    B = beta (scale + 1) + shift, |B| <= 8 - distinct (A, B) pairs within a vector, between neighbouring vectors and between samples."""
    c = torch.arange(C)
    b = torch.arange(B)[:, None]
    gamma = (1 + c % 2).double()
    beta = (c % 5 - 2).double()
    scale = ((b + c // 2) % 2).double()
    shift = ((3 * c + 5 * b) % 9 - 4).double()
    return gamma, beta, scale, shift


@functools.lru_cache(maxsize=None)
def gn_case(shape: GnShape) -> GnCase:
    """x = 40..47 (then t = A x + B in [32, 196]: SiLU is the identity) or -111..-104 (t in [-452, -96]: SiLU is -0), a quarter of
    the elements in the zero region; residual -8..8.  Expected A x + B, respectively 0, plus the residual: integers up to 204."""
    B, hw, C = shape.B, shape.hw, shape.C
    q, c = torch.arange(PERIOD)[:, None], torch.arange(C)[None, :]
    h = _hash(q, c)
    zero = (h >> 8) % 4 == 0
    x = torch.where(zero, -(104 + h % 8), 40 + h % 8).double()
    res = ((_hash(c, q) % 17) - 8).double() if shape.residual else None
    gamma, beta, scale, shift = gn_coefs(C, B)
    A = (gamma * (scale + 1))[:COEF_PERIOD]
    Bc = (beta * (scale + 1) + shift)[:COEF_PERIOD]
    if B < COEF_PERIOD:                                       # rows b >= B are never used
        A, Bc = A[:B], Bc[:B]
    t = A[:, None, :] * x[None] + Bc[:, None, :]
    assert bool(((t >= SILU_ID_MIN) | (t <= SILU_ZERO_MAX)).all()) and float(t.abs().max()) < 2.0 ** 24
    want = torch.where(t >= SILU_ID_MIN, t, torch.zeros_like(t)) + (res[None] if shape.residual else 0)
    bound = 256 if shape.bf16 else 2.0 ** 24
    for v in (x, want) + ((res,) if shape.residual else ()):
        assert float(v.abs().max()) < bound and bool((v == v.round()).all())
    s1, s2 = unit_stats(hw, C // shape.groups)
    partial = torch.tensor([s1, s2], dtype=torch.float32).expand(B, shape.groups, 1, 2).contiguous()
    return GnCase(shape, x.float(), None if res is None else res.float(), gamma.float(), beta.float(),
                  torch.cat((scale, shift), 1).float().contiguous(), partial, A, Bc, want.float())


def gn_want(case: GnCase, b0=0, nb=None):
    """Expected output [nb, hw, C] (fp32, exact) of samples b0 .. b0 + nb, and the input and residual of the same samples."""
    s = case.shape
    nb = s.B - b0 if nb is None else nb
    r = torch.arange(b0 * s.hw, (b0 + nb) * s.hw)
    bb = (r // s.hw) % case.want_table.shape[0]
    want = case.want_table[bb, r % PERIOD].reshape(nb, s.hw, s.C)
    x = case.base_x[r % PERIOD].reshape(nb, s.hw, s.C)
    res = None if case.base_res is None else case.base_res[r % PERIOD].reshape(nb, s.hw, s.C)
    return want, x, res


def gn_reference(x, res, A, Bc, *, vector_shift=0, sample0_coefs=False, drop_residual=False, N=4):
    """float64 silu(A x + B) + residual on [nb, hw, C] with coefficients [nb, C]; the keyword arguments are the mutants."""
    A, Bc = A.double(), Bc.double()
    if vector_shift:
        A, Bc = torch.roll(A, -N * vector_shift, 1), torch.roll(Bc, -N * vector_shift, 1)
    if sample0_coefs:
        A, Bc = A[:1].expand_as(A), Bc[:1].expand_as(Bc)
    t = A[:, None, :] * x.double() + Bc[:, None, :]
    y = t / (1 + torch.exp(-t))
    y = torch.where(t <= SILU_ZERO_MAX, torch.zeros_like(y), y)
    return y + (res.double() if res is not None and not drop_residual else 0)


GN_MUTANTS = {"coefficients_of_the_next_vector": dict(vector_shift=1), "coefficients_of_sample_0": dict(sample0_coefs=True),
              "residual_dropped": dict(drop_residual=True)}


def assert_exact(got: torch.Tensor, want: torch.Tensor, what=""):
    """Bit for bit, -0 == +0 (comparison as numbers), no NaN."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    n = int(bad.sum())
    if n:
        i = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r" % (
            what, n, got.numel(), i, float(got[tuple(i)]), float(want[tuple(i)])))


def assert_guards(buf: torch.Tensor, n: int, sentinel: float, what=""):
    """buf = [GUARD | n elements | GUARD]: both bands still hold the sentinel."""
    assert buf.numel() == n + 2 * GUARD
    assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all()), what + ": guard band written"


# ------------------------------------------------------------------------------------------------ 2. SiLU over its whole range
SWEEP_POINTS = (0.0, 2.0 ** -130, 1e-30, 1e-3, 0.5, 1.0, 5.0, 16.6, 17.0, 20.0, 40.0, 87.0, 88.7, 89.0, 95.0, 103.0, 104.0, 1e4)


@functools.lru_cache(maxsize=None)
def silu_sweep(bf16: bool) -> torch.Tensor:
    """fp32 pre-activations of both signs: the named points and 4096 log-spaced magnitudes from 2^-140 to 2^14, padded with
    zeros to a whole number of 128-channel pixels; rounded to bf16 first in bf16 mode."""
    mags = torch.cat((torch.tensor(SWEEP_POINTS, dtype=torch.float64), torch.logspace(-140, 14, 4096, base=2.0, dtype=torch.float64)))
    t = torch.cat((mags, -mags)).float()
    t = torch.cat((t, torch.zeros(-t.numel() % 128)))
    return t.to(torch.bfloat16).float() if bf16 else t


def silu64(t):
    t = t.double()
    return t / (1 + torch.exp(-t))


def silu_tolerance(t: torch.Tensor, extra: torch.Tensor = None) -> torch.Tensor:
    """Per element.  The oracle's own fp32 evaluation (F.silu in fp32) against float64 is measured per binade of |t| - one
    distance over the whole sweep would be the rounding of the largest value, 1e4, and say nothing about the small ones - as the
    largest absolute distance of the binade, times MARGIN, with the floor of FLOOR_ULPS ulp of the binade's largest |silu| and of
    4 fp32 denormal steps; ``extra`` (a split site's emulation distance, elementwise) adds its largest value of the binade; a bf16 site adds its storage rounding (bf16_store_bound, in silu_miss).  The binades where fp32 exp(-t) overflows
    while silu(t) is still a normal number (t in (-104, -88.7)) carry the fp32 evaluation's own miss there, 2.6e-37."""
    ref = silu64(t)
    e32 = (torch.nn.functional.silu(t.float()).double() - ref).abs()
    binade = torch.where(t == 0, torch.full_like(t, -200.0), torch.floor(torch.log2(t.abs().double().clamp_min(2.0 ** -160))).float())
    key = binade * 2 + (t < 0).float()
    tol = torch.zeros_like(ref)
    for k in key.unique():
        m = key == k
        top = float(ref[m].abs().max())
        tol[m] = max(MARGIN * float(e32[m].max()), FLOOR_ULPS * ulp32(top), 4 * 2.0 ** -149) + (float(extra[m].max()) if extra is not None else 0.0)
    return tol


def silu_miss(got: torch.Tensor, t: torch.Tensor, bf16_store: bool, extra: torch.Tensor = None) -> float:
    """The largest |got - silu64(t)| / tolerance; infinite where got is not finite (the reference is finite everywhere)."""
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got.double() - silu64(t)).abs() / (silu_tolerance(t, extra) + (bf16_store_bound(silu64(t)) if bf16_store else 0))).max())


SILU_MUTANTS = {
    "overflow_not_caught": lambda t: torch.where(t < -88.0, torch.full_like(t, float("nan")), silu64(t)),      # t * (1 / inf) done as t * 0 * inf
    "tanh_sigmoid_clamped": lambda t: t * (0.5 * torch.tanh(0.5 * t.clamp(-15, 15)) + 0.5),                    # saturating too early: silu(-20) = 0
    "hard_swish": lambda t: t * (t / 6 + 0.5).clamp(0, 1),
}


# The SiLU sites inside the convolutions (t * rcp(1 + __expf(-t)), conv_common.hpp / conv3x3_mx2.hip / the conv1x1 epilogues), each
# seeing the sweep through A = 1, B = 0.  "gnin": the producer's GroupNorm + SiLU applied while the input is staged,
# conv(silu(a x + b)) with centre-tap selection weights of 1.0 and no bias: the convolution adds nothing but its operand rounding.
# "tail": out = silu(a h + b) + conv(x) with 1x1 selection weights and x = 0: the convolution adds exactly 0.
# impl: the implementation number of srgd_k_conv2d_timed; split: the operand arithmetic whose emulation distance the site is granted.
CONV_SITES = {
    "conv3x3_bf16_gnin": dict(impl=5, bf16=True, ks=3, kind="gnin", split=None),
    "conv3x3_split_gnin": dict(impl=11, bf16=False, ks=3, kind="gnin", split="f16x3"),
    "conv3x3_mx2_gnin": dict(impl=15, bf16=False, ks=3, kind="gnin", split="f16mx2"),
    "conv1x1_bf16_tail": dict(impl=3, bf16=True, ks=1, kind="tail", split=None),
    "conv1x1_split_tail": dict(impl=10, bf16=False, ks=1, kind="tail", split=None),
}
SITE_SHAPE = (1, 128, 8, 32)                # NCHW: 128 -> 128 channels, 256 pixels - eligible for every one of the five kernels
F16_MAX = 65504.0


@functools.lru_cache(maxsize=None)
def site_case(site):
    """-> (t [32768] fp32, x NCHW, w [128, 128, ks, ks], extra or None): the sweep repeated to fill the tensor - clamped to the f16
    range for the split sites, whose operands saturate there -, selection weights of 1.0, and for a split site the elementwise
    distance of oracle/split_emulation.py's arithmetic on float32(silu64(t)) from that value."""
    from oracle import split_emulation as SE
    c = CONV_SITES[site]
    n = SITE_SHAPE[0] * SITE_SHAPE[1] * SITE_SHAPE[2] * SITE_SHAPE[3]
    base = silu_sweep(c["bf16"])
    t = base.repeat(-(-n // base.numel()))[:n].clone()
    if c["split"]:
        t = t.clamp(-F16_MAX, F16_MAX)
    x = t.reshape(SITE_SHAPE)
    C = SITE_SHAPE[1]
    w = torch.zeros(C, C, c["ks"], c["ks"])
    w[torch.arange(C), torch.arange(C), c["ks"] // 2, c["ks"] // 2] = 1.0
    extra = None
    if c["split"]:
        act = silu64(t).float().reshape(SITE_SHAPE)
        emu = SE.split_conv2d(act, w, None, padding=1) if c["split"] == "f16x3" else SE.mixed_split_conv2d(act, w, None, padding=1, mode="f16mx2")
        extra = (emu.double() - act.double()).abs().reshape(-1)
    return t, x, w, extra


# ------------------------------------------------------------------------------------------------ 3. rms_norm: the launch model
@dataclass(frozen=True)
class RmsLaunch:
    N: int
    vpp: int
    L: int                 # lanes per pixel
    v_trips: int           # ceil(vpp / L): trips of the v loop of the busiest lane
    ragged: bool           # some lanes make fewer trips than others
    pix_per_trip: int      # pixels the whole grid takes per trip of the grid-stride loop
    grid: int
    pixel_trips: int


def rms_launch(npix, C, bf16) -> RmsLaunch:
    """rms_norm's launch, restated from its comment: "L lanes cooperate on one pixel (L = largest power of two <= min(64, C / vec))",
    256 / L pixels per block, at most 256 * 32 = 8192 blocks; beyond 8192 * 256 / L pixels the grid-stride loop makes another trip."""
    N = 8 if bf16 else 4
    assert C % N == 0
    vpp = C // N
    L = 1
    while L * 2 <= min(64, vpp):
        L *= 2
    ppb = 256 // L
    grid = min(-(-npix // ppb), 8192)
    return RmsLaunch(N, vpp, L, -(-vpp // L), vpp % L != 0, grid * ppb, grid, -(-npix // (grid * ppb)))


def gain(C):
    """Distinct per channel, dyadic, 8 significant bits (an exact bf16): (128 + c % 128) 2^(c // 128 - 7 - 3), 2^-3 .. 2^5."""
    c = torch.arange(C)
    return ((128 + c % 128).double() * 2.0 ** (c // 128 - 10).double())


@dataclass(frozen=True)
class RmsShape:
    npix: int
    C: int
    bf16: bool

    @property
    def id(self):
        return "%s_C%d_npix%d" % ("bf16" if self.bf16 else "fp32", self.C, self.npix)


def second_trip_npix(C, bf16):
    return 8192 * (256 // rms_launch(1, C, bf16).L) + 3


# C = 4^k: L = 4, 16, 64 and the four-trip v loop at C / N = 256 (fp32); bf16: L = 2, 8, 32, 64 (two trips).  1500 pixels: more than
# one period of the data and several blocks.  Then the second trip of the grid-stride loop: 8192 * 256 / L + 3 pixels at the smallest
# tensor per type (fp32 C = 16, bf16 C = 32: L = 4, 524 291 pixels) and at L = 64 (fp32 C = 256: 32 771 pixels).
RMS_EXACT_SHAPES = tuple(RmsShape(1500, C, bf16) for bf16 in (False, True) for C in (16, 64, 256, 1024)) + (
    RmsShape(second_trip_npix(16, False), 16, False), RmsShape(second_trip_npix(32, True), 32, True),
    RmsShape(second_trip_npix(256, False), 256, False))


@dataclass
class RmsExact:
    base_x: torch.Tensor       # fp32 [PERIOD, C]
    base_res: torch.Tensor     # fp32 [PERIOD, C]
    g: torch.Tensor            # fp32 [C]
    want: torch.Tensor         # fp32 [PERIOD, C], without the residual: +-g_c 2^i, or 0
    want_res: torch.Tensor     # with it (bf16: rounded once, as the store does)


@functools.lru_cache(maxsize=None)
def rms_exact(C, bf16) -> RmsExact:
    """Row q of the period: i = q % (imax + 1) with 4^imax <= min(C, 64), m = C / 4^i entries +-a, a = 2^((2 q) % 7 - 3) - so that the
    norm sqrt(m) a of a row differs from its neighbours' (i + 1 or i - imax against a * 4 or a / 32) -, at the channels
    (3 q) % 4^i + 4^i u - spread over every lane and every trip of the v loop -, signs by a hash.  Residual: n g_c 2^i with
    n in -2..2, so that the fp32 sum (s + n) g_c 2^i is exact; a bf16 store rounds it once."""
    n = int(math.log2(C))
    assert 2 ** n == C
    imax = min(n // 2, 3)
    q, c = torch.arange(PERIOD)[:, None], torch.arange(C)[None, :]
    i = q % (imax + 1)
    step = 4 ** i
    a = 2.0 ** ((2 * q) % 7 - 3).double()
    on = c % step == (3 * q) % step
    h = _hash(q, c)
    sign = torch.where(h % 2 == 0, 1.0, -1.0).double()
    x = torch.where(on, sign * a, torch.zeros((), dtype=torch.float64))
    g = gain(C)
    want = torch.where(on, sign * g[None] * 2.0 ** i.double(), torch.zeros((), dtype=torch.float64))
    res = ((h >> 4) % 5 - 2).double() * g[None] * 2.0 ** i.double()
    want_res = want + res
    for v in (x, g, res, want, want_res):
        assert torch.equal(v.float().double(), v)                      # exact in fp32
    for v in (x, g, want) if bf16 else ():
        assert torch.equal(v.to(torch.bfloat16).double(), v)           # inputs and the plain output exact in bf16
    if bf16:
        res = res.to(torch.bfloat16).double()                          # 3 g and 5 g have more than 8 bits ...
        want_res = (want + res).float().to(torch.bfloat16).double()    # ... the fp32 sum is exact, the store rounds once
        assert torch.equal((want + res).float().double(), want + res)
    return RmsExact(x.float(), res.float(), g.float(), want.float(), want_res.float())


def rms_reference(x, g, res=None, *, mutant=None, launch: RmsLaunch = None):
    """float64 x / max(||x||, 1e-12f) * g * sqrt(C) (+ residual) on [npix, C]; ``mutant`` names a wrong kernel."""
    x64, g = x.double(), g.double()
    npix, C = x.shape
    norm = x64.pow(2).sum(1, keepdim=True).sqrt()
    if mutant == "norm_of_the_next_pixel":
        norm = torch.roll(norm, -1, 0)
    elif mutant == "norm_of_the_previous_pixel":
        norm = torch.roll(norm, 1, 0)
    elif mutant == "norm_one_grid_stride_away":
        norm = torch.roll(norm, -(launch.pix_per_trip % npix), 0)
    elif mutant == "first_L_vectors_only":
        norm = x64[:, :launch.L * launch.N].pow(2).sum(1, keepdim=True).sqrt()
    if mutant == "gain_off_by_one_vector":
        g = torch.roll(g, -launch.N, 0)
    den = norm + EPS_NORM if mutant == "eps_added" else norm.clamp_min(EPS_NORM)
    den = torch.where(torch.isnan(norm), norm, den)                    # clamp_min keeps a NaN, as the kernel's max_keep_nan does
    y = x64 / den * g[None] * (1.0 if mutant == "sqrt_C_missing" else math.sqrt(C))
    return y + (res.double() if res is not None else 0)


RMS_MUTANTS = ("norm_of_the_next_pixel", "norm_of_the_previous_pixel", "norm_one_grid_stride_away", "gain_off_by_one_vector",
               "sqrt_C_missing", "eps_added", "first_L_vectors_only")

# ------------------------------------------------------------------------------------------------ 4. rms_norm: ragged shapes, float64
# C / N no power of two: the v loop is ragged (C = 24: 6 vectors over L = 4 lanes in fp32, 3 over L = 2 in bf16; 136 / 4 = 34 = 272 / 8
# over L = 32).  131 pixels: several blocks, a ragged last one.
RMS_RAGGED = tuple(RmsShape(131, C, False) for C in (24, 48, 96, 136)) + tuple(RmsShape(131, C, True) for C in (24, 48, 96, 272))


@dataclass
class RmsValues:
    x: torch.Tensor            # fp32 [npix, C] (bf16 mode: bf16-exact)
    res: torch.Tensor
    g: torch.Tensor
    want: torch.Tensor         # float64, with the residual
    want_plain: torch.Tensor   # without
    tol: float                 # scalar part of the bound, for both
    e32: float


def _tolerance(x, g, res, want, want_plain):
    C = x.shape[1]
    o32 = O.rms_norm(x[:, :, None, None], g.view(1, C, 1, 1))[:, :, 0, 0]
    e32 = max(distance(o32 + res, want), distance(o32, want_plain))
    return max(MARGIN * e32, FLOOR_ULPS * ulp32(float(want.abs().max()))), e32


@functools.lru_cache(maxsize=None)
def rms_ragged(shape: RmsShape) -> RmsValues:
    """Gaussian rows scaled by 2^+-20 per pixel, gains 1 + 0.1 N, residual N(0, 1); bf16 mode: rounded to bf16 first."""
    gen = torch.Generator().manual_seed(900 + shape.C + int(shape.bf16))
    p = torch.arange(shape.npix)[:, None]
    x = torch.randn(shape.npix, shape.C, generator=gen) * 2.0 ** ((p % 3 - 1) * 20).float()
    res = torch.randn(shape.npix, shape.C, generator=gen)
    g = 1 + 0.1 * torch.randn(shape.C, generator=gen)
    if shape.bf16:
        x, res = x.to(torch.bfloat16).float(), res.to(torch.bfloat16).float()
    want, plain = rms_reference(x, g, res), rms_reference(x, g)
    tol, e32 = _tolerance(x, g, res, want, plain)
    return RmsValues(x, res, g, want, plain, tol, e32)


def within(got, want, tol, bf16) -> float:
    """The largest |got - want| / (tol + half a bf16 step at the reference's bf16 rounding for a bf16 store); NaN must sit where want has it and
    nowhere else."""
    got, want = got.double(), want.double()
    if not torch.equal(torch.isnan(got), torch.isnan(want)):
        return float("inf")
    ok = ~torch.isnan(want)
    if not bool(torch.isfinite(got[ok]).all()):
        return float("inf")
    bound = tol + (bf16_store_bound(want[ok]) if bf16 else 0)
    return float(((got[ok] - want[ok]).abs() / bound).max())


# ------------------------------------------------------------------------------------------------ 5. rms_norm: edge rows
EDGE_ROWS = ("zero", "norm_2^-58", "squares_underflow", "norm_2^-40", "nan", "plain")


@functools.lru_cache(maxsize=None)
def rms_edges(C, bf16):
    """One pixel per edge, ordinary pixels between them (a NaN must not reach them), expected by the reference's fp32 semantics
    x / max(||x||, 1e-12) in float64:
      zero               an all-zero row -> zeros
      norm_2^-58         four entries of 2^-59: the clamp decides, x sqrt(C) / 1e-12 g
      squares_underflow  entries of 2^-80: their squares are 0 in fp32, the same expression
      norm_2^-40         four entries of 2^-41: norm 9.1e-13, just under the clamp - where adding eps instead of clamping is off by 1.9
      nan                one NaN channel: the whole pixel is NaN, no other pixel is
    Tolerance 4 ulp of each element (plus the bf16 store's half step)."""
    npix = 9
    gen = torch.Generator().manual_seed(77 + C)
    x = torch.randn(npix, C, generator=gen)
    g = gain(C).float()
    x[1] = 0
    x[2] = 0
    x[2, [0, C // 2, C // 2 + 1, C - 1]] = torch.tensor([1.0, -1.0, 1.0, -1.0]) * 2.0 ** -59
    x[4] = torch.where(torch.arange(C) % 3 == 0, 2.0 ** -80, -(2.0 ** -80))
    x[5] = 0
    x[5, [1, C // 2, C // 2 + 2, C - 2]] = torch.tensor([1.0, 1.0, -1.0, -1.0]) * 2.0 ** -41
    x[7, C // 3] = float("nan")
    if bf16:
        x = x.to(torch.bfloat16).float()
    rows = {"zero": 1, "norm_2^-58": 2, "squares_underflow": 4, "norm_2^-40": 5, "nan": 7, "plain": 0}
    # the kernel's fp32 sum of squares of the underflow row is 0: the clamp decides there too (in float64 it is 2^-160 C, far below)
    want = rms_reference(x, g)
    return x, g, want, rows


def edge_miss(got, want, bf16) -> float:
    """Elementwise: 4 ulp of the expected value (at least 4 denormal steps), plus the bf16 store's half step."""
    got, want = got.double(), want.double()
    if not torch.equal(torch.isnan(got), torch.isnan(want)):
        return float("inf")
    ok = ~torch.isnan(want)
    w = want[ok]
    if not w.numel():
        return 0.0
    ulp = 2.0 ** (torch.floor(torch.log2(w.abs().clamp_min(2.0 ** -126))) - 23)
    return float(((got[ok] - w).abs() / (FLOOR_ULPS * ulp + (bf16_store_bound(w) if bf16 else 0))).max())


# ------------------------------------------------------------------------------------------------ 6. the RMSNorm folded into conv1x1_split
REL_FP32 = 2.0 ** -21           # as attention_cases.REL_FP32: one reciprocal and one multiply, doubled


@dataclass(frozen=True)
class Folded:
    kind: str                   # "pre": out = W . RMSNorm_g(x);  "post": out = RMSNorm_g(W . x) + residual
    Cin: int
    Cout: int
    B: int
    N: int

    @property
    def id(self):
        return "%s_Cin%d_Cout%d_B%d_N%d" % (self.kind, self.Cin, self.Cout, self.B, self.N)

    @property
    def tiles(self):
        """conv1x1_split.hip: T = m-tiles x n-tiles of 256 pixels x 128 output channels; the grid is persistent, "at most one
        workgroup per CU" (256 on an MI355X): with T above that a workgroup takes tiles v, v + gridDim.x, ..."""
        return self.B * self.N // 256 * (self.Cout // 128)


# N = 256 with B = 8: a tile per sample; the two large ones have T = 288 and 320 tiles, more than the 256 CUs
FOLDED = (Folded("pre", 128, 384, 8, 256), Folded("pre", 256, 384, 8, 256), Folded("pre", 256, 384, 2, 12288),
          Folded("post", 128, 128, 8, 256), Folded("post", 256, 128, 8, 256), Folded("post", 128, 128, 2, 40960))
CUS = 256


def folded_selection(f: Folded) -> torch.Tensor:
    """Output channel o reads input channel (5 o + 3) % Cin: selection weights of 1.0, a bijection when Cout == Cin."""
    return (5 * torch.arange(f.Cout) + 3) % f.Cin


def folded_weights(f: Folded) -> torch.Tensor:
    w = torch.zeros(f.Cout, f.Cin)
    w[torch.arange(f.Cout), folded_selection(f)] = 1.0
    return w


def folded_exact(f: Folded) -> bool:
    """Bit for bit where every intermediate is exact: the pre-norm at Cin = 256.  The folded weight g_c sqrtf(256) has 8 significant
    bits - an exact f16 after the layer's power-of-two weight scale -, x = +-2^e is an exact f16, an output is ONE non-zero product,
    and 1 / ||x|| is a power of two.  At Cin = 128, sqrtf(128) is not dyadic; the post-norm divides by the norm of 128 channels,
    sqrt(2) 2^k: those are held to REL_FP32."""
    return f.kind == "pre" and f.Cin == 256


@functools.lru_cache(maxsize=None)
def folded_case(f: Folded):
    """-> (base_x [PERIOD, Cin], gain [C of the norm], W [Cout, Cin], base_res or None, base_want float64 [PERIOD, Cout], base_mag):
    the exact rows of rms_exact; base_mag = |normalised term| + |residual|, what REL_FP32 is relative to."""
    e = rms_exact(f.Cin, False)
    sel = folded_selection(f)
    if f.kind == "pre":
        want = rms_reference(e.base_x, e.g)[:, sel]
        if folded_exact(f):
            assert distance(want, e.want[:, sel]) <= 2.0 ** -50 * float(want.abs().max())
            want = e.want[:, sel].double()
        return e.base_x, e.g, folded_weights(f), None, want, want.abs()
    g = gain(f.Cout).float()
    res = rms_exact(f.Cout, False).base_res
    y = e.base_x[:, sel]
    normed = rms_reference(y, g)
    return e.base_x, g, folded_weights(f), res, normed + res.double(), normed.abs() + res.double().abs()


def folded_miss(got, want, mag, exact: bool) -> float:
    """exact: the number of differing elements; otherwise the largest |got - want| / (REL_FP32 * mag), zeros exact."""
    got, want = got.double(), want.double()
    if exact:
        return float((got != want).sum())
    if not bool(torch.isfinite(got).all()) or bool((got[mag == 0] != 0).any()):
        return float("inf")
    ok = mag > 0
    return float(((got[ok] - want[ok]).abs() / (REL_FP32 * mag[ok])).max())
