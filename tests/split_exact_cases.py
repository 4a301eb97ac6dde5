"""Inputs with NON-ZERO lo halves in both operands for every split-operand convolution kernel, their exact outputs, and the
conditions and assertions that go with them.

Pure torch on the CPU; test infrastructure only (used by tests/test_split_exact_gpu.py, which feeds the tensors to the HIP kernels
through the kernel-level C ABI, and by tests/test_split_exact_cases_cpu.py, which proves every condition below and shows that
torch.equal rejects eleven subtly wrong split convolutions).  The shapes are those of tests/conv_exact_cases.py; its integer data
leave every lo half zero, so the lo image of the activations (split8), the lo tile of every packed weight unit, the power-of-two
weight scale on non-integers and the two cross products are pinned here.

The arithmetic under test (srgd_amd/csrc/conv3x3_split.hip, oracle/split_emulation.py):
    x = x_hi + x_lo,  w * s = w_hi + w_lo,  acc = sum x_hi * w_hi + sum x_lo * w_hi + sum x_hi * w_lo  (fp32),  out = acc / s + bias

The data, f16 halves (F = 2^-14):
    x = a + p * F      a in {+-1, +-2}, p in {-3..3}            ->  x_hi = a,        x_lo = p * F
    w = c + d * F      c in {+-1},      d in {+-1..+-3}, or w = 0  ->  s = 2^10,  w_hi = +-1024,  w_lo = d * 2^-4
No integer part is zero (a zero one would move the fraction into the hi half); no kept weight has d = 0 (a subset of {-3..3}: where a
position keeps one weight per n-tile, as under GroupNorm-in-staging, a zero d would leave that position of the lo tile unseen).  The exponent is -14 and not -13 because just below
a power of two the f16 ulp halves: 1 - 3 * 2^-13 does not split this way.  Every term of the three sums is a multiple of
q = 2^-4, and the weights are thinned by structural zeros until, for every output element,
    sum |x_hi * w_hi| + sum |x_lo * w_hi| + sum |x_hi * w_lo|  <  2^BUDGET_BITS * q.
Any partial sum in any order is bounded by that absolute sum, fp32 holds 24 bits: with BUDGET_BITS = 22 the three-term sum is
exact in fp32 in every summation order, fragment layout and tiling, with two bits to spare (nobody has measured whether the matrix
core keeps all 24 bits when it adds small products to a much larger accumulator).  The kernel must then equal the float64
evaluation of the same three terms bit for bit.  acc / s is a multiple of 2^-14 below 2^8, so acc / s + bias (an integer bias,
|b| <= 4) is exact as well.  bf16 halves (s = 1): the same with F = 2^-11 = q; the budget is then 2^11 in absolute terms, which dense
weights keep up to K = 1021 - the two widest halo cases (K = 1152 and 3456) are thinned like the f16 ones.
BUDGET_BITS is the designed 22: on an MI355X every split kernel equals the reference bit for bit at it (absolute sums up to 0.86 of
the budget), so it was not lowered.

Thinning: per 128-channel n-tile every output channel keeps the same number n of non-zero weights (n = the budget divided by the
largest absolute value one product can contribute; about 127 for f16: density 0.2 at K = 576, 0.035 at K = 9 * 384); their
positions are dealt from shuffled decks of all K (tap, input channel) positions, so every position still meets a non-zero weight in
some output channel of every n-tile (random thinning at these densities would leave hundreds of positions untested).

Epilogues:
  up       bias = 32 + ceil(max|conv|) + {0..4}; SiLU is the identity for ANY argument >= 32 (1 + exp(-x) rounds to 1 in fp32)
  residual integer residuals; the sums stay fp32-exact
  tail     integer tail data as in conv_exact_cases (an fp32 epilogue): out = conv + silu(a * h + 64)
  staging  conv(silu(a_c * x + b_c)), x = +-1 + p * F, (a_c, b_c) in {(2, 38), (2, 42), (4, 40)}: v = a_c * x + b_c is an exact fma,
           v >= 32, its hi half is 36, 40 or 44 (exact in e4m3 under a power-of-two block scale: impl 15) and its lo half is
           a_c * p * F.  Five non-zero weights per output channel is what the budget then leaves; the deck keeps every position covered.
No GroupNorm partial sums here (sums of squares of fractional values are not exact; that epilogue reads finished accumulators and
is pinned on integers).

The 2^-10 cases: the same activations times 2^-10.  x_hi = a * 2^-10 is a normal f16, every x_lo = p * 2^-24 an f16 SUBNORMAL;
acc is the base case's acc times 2^-10, exactly, so a flush of f16 subnormals in the conversion or in the MFMA shows as a bitwise
difference.  acc / s is then a multiple of 2^-24 and the bias add is the one rounding of the case: the expected value is the
float64 sum rounded to fp32 once, which is what a correctly rounded fp32 add or fma gives (the multiplication by 1 / s is exact).
"""
import collections
import functools
import math
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle.split_emulation import halves, weight_scale
from tests import conv_exact_cases as X
from tests.conv_exact_cases import SILU_MIN, TAIL_B, Spec

BUDGET_BITS = 22                          # the exactness budget, in bits above the common quantum q of the three terms (designed: 22; fp32 holds 24)
FRAC = {"f16": 2.0 ** -14, "bf16": 2.0 ** -11}
QUANTUM = {"f16": 2.0 ** -4, "bf16": 2.0 ** -11}      # of the terms of acc (f16: after the weight scale 2^10)
W_SCALE = {"f16": 2.0 ** 10, "bf16": 1.0}
P_MAX = 3                                 # |p|, |d| <= P_MAX
X_SCALE = 2.0 ** -10                      # the subnormal cases
N_TILE = 128
STAGING_COEF = ((2.0, 38.0), (2.0, 42.0), (4.0, 40.0))          # (a_c, b_c): hi of a_c * (+-1) + b_c in {36, 40, 44}


def budget(kind):
    """The bound on the absolute sum of the terms of one output element (in the units of acc)."""
    return 2.0 ** BUDGET_BITS * QUANTUM[kind]


def _x_hi_max(spec):
    return max(abs(a) + b for a, b in STAGING_COEF) if spec.staging else 2.0


def products_per_output(spec, kind):
    """How many non-zero weights one output channel keeps: the budget over the largest absolute value one product can add."""
    s, frac = W_SCALE[kind], FRAC[kind]
    xh = _x_hi_max(spec)
    xl = P_MAX * frac * (max(a for a, _ in STAGING_COEF) if spec.staging else 1.0)
    per_product = xh * s + xl * s + xh * P_MAX * frac * s
    return min(spec.K, int(budget(kind) / per_product))


def budget_density(spec, kind):
    """The share of non-zero weights (in the manner of conv_exact_cases.stats_density)."""
    return products_per_output(spec, kind) / spec.K


@dataclass
class Case:
    spec: Spec
    kind: str                             # "f16" | "bf16": the halves of the kernel the data are designed for
    scaled: bool                          # the activations times X_SCALE
    x0: torch.Tensor
    x1: torch.Tensor
    w: torch.Tensor
    bias: torch.Tensor
    residual: torch.Tensor
    tail: tuple
    coef: tuple
    density: float
    want: torch.Tensor = None             # float64
    silu_args: torch.Tensor = None

    @property
    def name(self):
        return "%s-%s%s" % (self.spec.name, self.kind, "-x2m10" if self.scaled else "")


Terms = collections.namedtuple("Terms", "xh xl wh wl s hh lh hl pad act raw")
Ref = collections.namedtuple("Ref", "out pre acc silu_args")


def _conv(x, w, pad):
    return F.conv2d(x.double(), w.double(), None, padding=pad)


def conv_input(c):
    """(what the convolution sums over as fp32: the activated, unshuffled input; the raw input in the same layout; the padding)."""
    s = c.spec
    raw = c.x0 if c.x1 is None else torch.cat((c.x0, c.x1), 1)
    act = raw
    if s.staging:
        v = c.coef[0].double()[:, :, None, None] * raw.double() + c.coef[1].double()[:, :, None, None]
        act = v.float()                   # (exact: staging_value_is_an_exact_fma)
    if s.layer == "down":
        raw, act = F.pixel_unshuffle(raw, 2), F.pixel_unshuffle(act, 2)
    return act, raw, (1 if s.layer == "3x3" else 0)


def terms(c):
    """The halves of both operands and the three exact sums, float64.  Cached on the case: nobody may write to them."""
    if getattr(c, "_terms", None) is None:
        act, raw, pad = conv_input(c)
        s = weight_scale(c.w, c.kind)
        xh, xl = halves(act, c.kind)
        wh, wl = halves(c.w * s, c.kind)
        c._terms = Terms(xh, xl, wh, wl, s, _conv(xh, wh, pad), _conv(xl, wh, pad), _conv(xh, wl, pad), pad, act, raw)
    return c._terms


MUTANTS = ("drop_xlo_whi_last_tap_last_chunk", "drop_xhi_wlo_one_ntile", "add_xlo_wlo", "xlo_whi_twice", "xlo_wlo_for_xlo_whi",
           "swap_lo_in_piece", "shift_lo_column", "zero_lo_source1", "lo_before_activation", "scale_bias", "flush_subnormal_xlo")


def mutant_applies(c, mutant):
    s = c.spec
    return {"zero_lo_source1": s.C1 > 0, "lo_before_activation": s.staging, "flush_subnormal_xlo": c.scaled and c.kind == "f16",
            "scale_bias": W_SCALE[c.kind] != 1.0,                     # bf16 halves: there is no scale
            # f16 "up" layers: the bias of 32 + max|conv| puts the ulp of every output at 2^-18 or above, the whole x_lo * w_lo sum
            # is about 2^-23 (it shows where |out| < 1, in about one output in seven of the other layers)
            "add_xlo_wlo": not (s.layer == "up" and c.kind == "f16")}.get(mutant, True)


def reference(c, mutant=None):
    """Ref in float64: the three terms on the halves of oracle.split_emulation.halves, / s, then the epilogue (SiLU taken as the
    identity: every argument is >= SILU_MIN).  `mutant`: one deliberate defect a kernel or a packer could have; None is the reference."""
    s = c.spec
    t = terms(c)
    pad = t.pad
    acc = t.hh + t.lh + t.hl
    bias = c.bias.double().view(1, -1, 1, 1)
    lo_variant = None                     # a replacement for x_lo in the x_lo * w_hi term
    if mutant == "drop_xlo_whi_last_tap_last_chunk":
        wm = torch.zeros_like(t.wh)
        wm[:, -32:, -1, -1] = t.wh[:, -32:, -1, -1]
        acc = acc - _conv(t.xl, wm, pad)
    elif mutant == "drop_xhi_wlo_one_ntile":                          # the last 128-channel n-tile
        lo_ch = (s.Cout - 1) // N_TILE * N_TILE
        acc = acc.clone()
        acc[:, lo_ch:] -= t.hl[:, lo_ch:]
    elif mutant == "add_xlo_wlo":
        acc = acc + _conv(t.xl, t.wl, pad)
    elif mutant == "xlo_whi_twice":
        acc = acc + t.lh
    elif mutant == "xlo_wlo_for_xlo_whi":
        acc = t.hh + _conv(t.xl, t.wl, pad) + t.hl
    elif mutant == "swap_lo_in_piece":                                # channels 1 and 2 of the first 8-channel piece; hi untouched
        idx = list(range(t.xl.shape[1]))
        idx[1], idx[2] = 2, 1
        lo_variant = t.xl[:, idx]
    elif mutant == "shift_lo_column":                                 # the lo image one column to the right, zero-filled
        lo_variant = torch.zeros_like(t.xl)
        lo_variant[..., 1:] = t.xl[..., :-1]
    elif mutant == "zero_lo_source1":
        lo_variant = t.xl.clone()
        lo_variant[:, s.C0 * (4 if s.layer == "down" else 1):] = 0
    elif mutant == "lo_before_activation":
        lo_variant = halves(t.raw, c.kind)[1]
    elif mutant == "flush_subnormal_xlo":
        lo_variant = torch.where(t.xl.abs() < 2.0 ** -14, torch.zeros_like(t.xl), t.xl)
    elif mutant not in (None, "scale_bias"):
        raise ValueError(mutant)
    if lo_variant is not None:
        acc = t.hh + _conv(lo_variant, t.wh, pad) + t.hl
    pre = (acc + bias) / t.s if mutant == "scale_bias" else acc / t.s + bias
    args = [t.act.double()] if s.staging else []
    out = pre
    if s.layer == "up":
        args.append(pre)
        out = F.pixel_shuffle(out, 2)
    if s.residual:
        out = out + c.residual.double()
    if s.tail:
        h, a, b = c.tail
        tl = a.double()[:, :, None, None] * h.double() + b.double()[:, :, None, None]
        args.append(tl)
        out = out + tl
    return Ref(out, pre, acc, torch.cat([v.reshape(-1) for v in args]) if args else None)


# ---------------------------------------------------------------------------------------------- the generator
def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _thin(g, cout, k, n):
    """[cout, k] mask with at most n non-zeros per row; per 128-row n-tile the positions are dealt from shuffled decks of all k."""
    if n >= k:
        return torch.ones(cout, k, dtype=torch.bool)
    mask = torch.zeros(cout, k, dtype=torch.bool)
    for lo in range(0, cout, N_TILE):
        rows = min(N_TILE, cout - lo)
        decks = torch.cat([torch.randperm(k, generator=g) for _ in range(-(-rows * n // k))])[:rows * n]
        mask[lo:lo + rows].scatter_(1, decks.reshape(rows, n), True)
    return mask


@functools.lru_cache(maxsize=None)
def build(spec, kind, scaled=False):
    """The seeded inputs of a case and its exact output.  Cached: nobody may write to the tensors.  Asserts the budget and the
    coverage (conditions, not measurements); tests/test_split_exact_cases_cpu.py proves the rest."""
    g = torch.Generator().manual_seed(11 + zlib.crc32(("%s/%s" % (spec.name, kind)).encode()) % 10007)
    s, frac = spec, FRAC[kind]

    def act(shape):
        mag = _randint(g, 1, 1 if s.staging else 2, shape)
        return ((2 * _randint(g, 0, 1, shape) - 1) * mag + _randint(g, -P_MAX, P_MAX, shape) * frac).float()

    x0 = act((s.B, s.C0, s.H, s.W))
    x1 = act((s.B, s.C1, s.H, s.W)) if s.C1 else None
    k = 3 if s.layer == "3x3" else 1
    cin = (s.C0 + s.C1) * (4 if s.layer == "down" else 1)
    shape = (s.Cout, cin, k, k)
    w = (2 * _randint(g, 0, 1, shape) - 1) + (2 * _randint(g, 0, 1, shape) - 1) * _randint(g, 1, P_MAX, shape) * frac    # d != 0
    n = products_per_output(s, kind)
    w = (w * _thin(g, s.Cout, cin * k * k, n).reshape(shape)).float()
    bias = _randint(g, -4, 4, (s.Cout,)).float()
    c = Case(s, kind, scaled, x0, x1, w, bias, None, None, None, float((w != 0).float().mean()))
    if s.staging:
        pick = torch.randint(0, len(STAGING_COEF), (s.B, s.C0), generator=g)
        table = torch.tensor(STAGING_COEF)
        c.coef = (table[pick, 0].contiguous(), table[pick, 1].contiguous())
    if scaled:
        c.x0 = x0 * X_SCALE
        c.x1 = None if x1 is None else x1 * X_SCALE
    if s.layer == "up":
        conv = reference(c).acc / W_SCALE[kind]
        c.bias = (SILU_MIN + math.ceil(float(conv.abs().max())) + _randint(g, 0, 4, (s.Cout,))).float()
    if s.residual:
        c.residual = _randint(g, -3, 3, (s.B, s.Cout, s.H, s.W)).float()
    if s.tail:
        c.tail = (_randint(g, -3, 3, (s.B, s.Cout, s.H, s.W)).float(), _randint(g, 1, 3, (s.B, s.Cout)).float(),
                  torch.full((s.B, s.Cout), float(TAIL_B)))
    ref = reference(c)
    c.want, c.silu_args = ref.out, ref.silu_args
    assert abs_sum_share(c) < 1.0, f"{c.name}: the absolute sum reaches {abs_sum_share(c):.3f} of the budget"
    assert covered(c), f"{c.name}: a (tap, input channel) position without a non-zero weight in some n-tile at density {c.density:.3f}"
    assert c.silu_args is None or float(c.silu_args.min()) >= SILU_MIN, c.name
    return c


# ---------------------------------------------------------------------------------------------- the conditions
def abs_sum_share(c):
    """max over the outputs of sum |x_hi w_hi| + sum |x_lo w_hi| + sum |x_hi w_lo|, as a share of the budget (must be < 1)."""
    t = terms(c)
    tot = _conv(t.xh.abs(), t.wh.abs(), t.pad) + _conv(t.xl.abs(), t.wh.abs(), t.pad) + _conv(t.xh.abs(), t.wl.abs(), t.pad)
    return float(tot.max()) / (budget(c.kind) * (X_SCALE if c.scaled else 1.0))


def covered(c):
    """Every (tap, input channel) position carries a non-zero weight - hi AND lo - for some output channel of each n-tile."""
    t = terms(c)
    both = (t.wh != 0) & (t.wl != 0)
    return all(bool(both[lo:lo + N_TILE].any(0).all()) for lo in range(0, c.spec.Cout, N_TILE))


def halves_are_the_designed_ones(c):
    """hi + lo reproduces every value, the hi halves are the integer parts (of x / X_SCALE, of w * s), the lo halves the fractions."""
    t = terms(c)
    xs = X_SCALE if c.scaled else 1.0
    x, ws = t.act.double() / xs, c.w.double() * t.s
    ok = torch.equal((t.xh.double() + t.xl.double()), t.act.double()) and torch.equal(t.wh.double() + t.wl.double(), ws)
    ok = ok and torch.equal(t.xh.double() / xs, x.round()) and bool((x.round() != 0).all()) and bool(((x - x.round()).abs() <= 4 * P_MAX * FRAC[c.kind]).all())
    ok = ok and torch.equal(t.wh.double(), (c.w.double().round() * t.s)) and t.s == W_SCALE[c.kind]
    q = QUANTUM[c.kind] * xs
    for term in (t.hh, t.lh, t.hl):
        ok = ok and torch.equal((term / q).round() * q, term)
    return ok


def lo_share(c):
    """(share of non-zero x_lo, share of non-zero w_lo among the non-zero weights)."""
    t = terms(c)
    return float((t.xl != 0).float().mean()), float((t.wl[t.wh != 0] != 0).float().mean())


def staging_value_is_an_exact_fma(c):
    t = terms(c)
    raw = c.x0
    a, b = c.coef[0][:, :, None, None], c.coef[1][:, :, None, None]
    v64 = a.double() * raw.double() + b.double()
    v32 = torch.addcmul(b.expand_as(raw), a.expand_as(raw), raw)        # fp32: a * x rounds nothing (a is 2 or 4), the add must not either
    hi_ok = bool(torch.isin(t.xh, torch.tensor([36.0, 40.0, 44.0])).all())
    lo_ok = torch.equal(t.xl.double(), a.double() * (raw.double() - raw.double().round()))
    return torch.equal(v32.double(), v64) and torch.equal(t.act.double(), v64) and float(v64.min()) >= SILU_MIN and hi_ok and lo_ok


def expected(c):
    return c.want.float()


def moved(a, b):
    """Share of the fp32 outputs in which two float64 results differ."""
    return float((a.float() != b.float()).float().mean())


def assert_output(c, got, what="the exact value"):
    """`got`: the kernel's output as fp32 NCHW on the CPU.  Returns nothing; raises with the count and the first index."""
    want = expected(c)
    assert got.shape == want.shape, (c.name, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        first = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError("%s: %d of %d elements differ from %s; first at [b, c, y, x] = %s: got %r, want %r" % (
            c.name, int(bad.sum()), bad.numel(), what, first, float(got[tuple(first)]), float(want[tuple(first)])))


# ---------------------------------------------------------------------------------------------- the table
_BY_NAME = {s.name: s for s in X.ALL}
HALO = [_BY_NAME[n] for n in ("halo_cpg16_one_patch", "halo_cpg32_two_sources", "halo_cpg16_B3", "halo_cpg128")]
HALO_IMPLS = [(6, "f16"), (8, "bf16"), (12, "f16"), (14, "f16")]      # (impl, the halves its data are designed for)
STAGING = list(X.STAGING)
STAGING_IMPLS = [(11, "f16"), (13, "f16"), (15, "f16")]
GENERIC = list(X.GENERIC)
GENERIC_IMPLS = [(7, "f16"), (9, "bf16")]
STREAM = list(X.STREAM)
STREAM_IMPLS = [(10, "f16")]
SCALED = [(_BY_NAME["halo_cpg16_one_patch"], [(6, "f16"), (12, "f16"), (14, "f16")]), (_BY_NAME["stream_plain"], STREAM_IMPLS)]    # f16 halves only: the subnormals are f16's
CROSS = _BY_NAME["halo_cpg16_one_patch"]                             # impl 6, 12 and 7 bitwise equal on it
MX_IMPLS = (14, 15)                                                   # the cross terms on MX-fp8 operands

FAMILIES = {"halo": (HALO, HALO_IMPLS), "staging": (STAGING, STAGING_IMPLS), "generic": (GENERIC, GENERIC_IMPLS),
            "stream": (STREAM, STREAM_IMPLS)}


def all_cases():
    """[(spec, kind, scaled, impls that run it)], one entry per distinct data set."""
    out = []
    for cases, impls in FAMILIES.values():
        for spec in cases:
            for kind in sorted({k for _, k in impls}):
                out.append((spec, kind, False, tuple(i for i, k in impls if k == kind)))
    for spec, impls in SCALED:
        for kind in sorted({k for _, k in impls}):
            out.append((spec, kind, True, tuple(i for i, k in impls if k == kind)))
    return out
