"""Inputs, expected bytes and assertions for every MX-fp8 quantisation site of the fp8 path.

Pure torch on the CPU; test infrastructure only (tests/test_mxfp8_exact_gpu.py feeds the tensors to the HIP kernels through the
kernel-level C ABI, tests/test_mxfp8_cases_cpu.py proves every condition stated below and shows that the assertions reject wrong
quantisers).  The expected bytes come from oracle/mxfp8.py (`MX.quantize`); `ref_quantize` below is a second, float64,
from-the-definition quantiser with knobs - its default setting is proved equal to the oracle on all the data here, its other
settings are the mutants.

Sites and their sections:
  1  quant_mxfp8 (quant_mxfp8.hip, plain)           `sweep`, `nonfinite`, `launch_case`
  2  gn_apply_silu_mxfp8 (the GroupNorm variant)     `gn_exact`, `gn_gaussian`
  3  the fused twins (mx_store_twin, mx_quant16_pair) `twin_conv_case`, `twin_gn_case`; expected twin = MX.quantize(stored bf16)
  4  the host weight quantisers                      `weight_case`, `onehot_3x3`, `read_back_3x3`, `assert_weights_read_back`
"""
import functools
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import mxfp8 as MX

Q_GUARD, S_GUARD, SENTINEL = 64, 16, 0xA5          # guard bands (bytes) around every GPU output buffer and their fill


# ------------------------------------------------------------------------------------------------ the reference quantiser + mutants
def scale_byte(amax, step="engine", log2="exact"):
    """E8M0 byte of a block maximum (any float dtype, NaN-free), from frexp - NOT from the bit fields the oracle and the kernels
    read.  step: "engine" (one step up when the mantissa exceeds 1.75), "ocp" (never), "ge" (at >= 1.75 - a mutant).
    log2 = "pow2_off": floor(log2) one too small at exact powers of two (a mutant of the host's frexp arithmetic)."""
    a = amax.double()
    m, ex = torch.frexp(a)                                   # a = m * 2^ex, m in [0.5, 1); a == 0 -> (0, 0); inf -> (inf, 0)
    fl = ex.to(torch.int64) - 1
    fl = torch.where(torch.isinf(a), torch.full_like(fl, 128), fl)
    m = torch.where(torch.isinf(a), torch.full_like(m, 0.5), m)
    if log2 == "pow2_off":
        fl = fl - (m == 0.5).to(torch.int64)
    over = {"engine": m * 2 > 1.75, "ocp": torch.zeros_like(m, dtype=torch.bool), "ge": m * 2 >= 1.75}[step]
    sb = (fl + 127 - 8 + over.to(torch.int64)).clamp(0, 254)
    return torch.where(a == 0, torch.zeros_like(sb), sb).to(torch.uint8)


def encode_e4m3(v, rounding="even", flush_sub=False):
    """float64 -> e4m3 'fn' bytes from the definition (1-4-3, bias 7, max 448, subnormals = multiples of 2^-9): saturating,
    NaN -> 0x7f.  rounding: "even" (the format's), "trunc", "away" (mutants); flush_sub: subnormal results become zero (mutant)."""
    v = v.double()
    nan = torch.isnan(v)
    a = torch.where(nan, torch.zeros_like(v), v.abs().clamp(max=448.0))
    _, ex = torch.frexp(a)
    e = (ex.to(torch.int64) - 1).clamp(min=-6)
    quantum = torch.ldexp(torch.ones_like(a), e - 3)
    r = a / quantum                                          # exact: a power of two
    n = {"even": torch.round, "trunc": torch.floor, "away": lambda t: torch.floor(t + 0.5)}[rounding](r)
    val = n * quantum
    if flush_sub:
        val = torch.where(val < 2.0 ** -6, torch.zeros_like(val), val)
    code = val.float().to(torch.float8_e4m3fn).view(torch.uint8)          # exact: val is a code point
    code = code | (torch.signbit(v).to(torch.uint8) << 7)
    return torch.where(nan, torch.full_like(code, 0x7F), code)


def ref_quantize(x, *, step="engine", rounding="even", flush_sub=False, amax_over="block", log2="exact"):
    """x [..., C] -> (q uint8 [..., C], s uint8 [..., C/32]).  amax_over: "block", "half" (the first 16 channels of the block
    only), "shifted" (channels 16..47: the partner half taken from the neighbouring block) - the last two are mutants."""
    shape = x.shape
    C = shape[-1]
    xd = x.double().reshape(-1, C)
    mag = torch.where(torch.isnan(xd), torch.zeros_like(xd), xd.abs())
    if amax_over == "half":
        amax = mag.reshape(-1, C // 32, 32)[..., :16].amax(-1)
    elif amax_over == "shifted":
        amax = torch.roll(mag, -16, dims=-1).reshape(-1, C // 32, 32).amax(-1)
    else:
        amax = mag.reshape(-1, C // 32, 32).amax(-1)
    sb = scale_byte(amax, step, log2)
    inv = torch.ldexp(torch.ones_like(amax), 127 - sb.to(torch.int64))
    q = encode_e4m3(xd.reshape(-1, C // 32, 32) * inv[..., None], rounding, flush_sub)
    return q.reshape(shape), sb.reshape(*shape[:-1], C // 32)


VALUE_MUTANTS = {                                           # name -> ref_quantize settings; every one is a wrong quantiser
    "ocp_rule": dict(step="ocp"),
    "step_up_at_ge_1.75": dict(step="ge"),
    "truncation": dict(rounding="trunc"),
    "round_half_away": dict(rounding="away"),
    "flush_e4m3_subnormals": dict(flush_sub=True),
    "amax_over_16_channels": dict(amax_over="half"),
    "amax_over_the_wrong_32": dict(amax_over="shifted"),
}


def scale_one_block_late(q, s):
    """the scale byte of block k stored at k + 1 (flat order)"""
    return q, torch.roll(s.reshape(-1), 1).reshape(s.shape)


def scale_of_previous_pixel(q, s):
    """pixel p's scale bytes stored at pixel p + 1"""
    return q, torch.roll(s.reshape(-1, s.shape[-1]), 1, dims=0).reshape(s.shape)


LAYOUT_MUTANTS = {"scale_one_block_late": scale_one_block_late, "scale_of_previous_pixel": scale_of_previous_pixel}


def decode_e4m3(q):
    return q.contiguous().view(torch.float8_e4m3fn).float()


def assert_bytes(got_q, got_s, want_q, want_s, what=""):
    """Bit equality of the scale bytes and the element bytes; a NaN element may carry either sign (0x7f / 0xff)."""
    got_q, got_s = got_q.reshape(want_q.shape), got_s.reshape(want_s.shape)
    bad = (got_s != want_s).nonzero()
    assert bad.numel() == 0, (what, "scale bytes", int(bad.shape[0]), bad[:4].tolist(),
                              [int(v) for v in got_s[tuple(bad[0])].reshape(-1)[:1]], [int(v) for v in want_s[tuple(bad[0])].reshape(-1)[:1]])
    nan = (want_q & 0x7F) == 0x7F
    differ = torch.where(nan, (got_q & 0x7F) != 0x7F, got_q != want_q)
    bad = differ.nonzero()
    assert bad.numel() == 0, (what, "element bytes", int(bad.shape[0]), bad[:4].tolist(), hex(int(got_q[tuple(bad[0])])),
                              hex(int(want_q[tuple(bad[0])])))


def assert_guards(buf, n, guard, what=""):
    """buf: the whole uint8 allocation [guard | n payload bytes | guard] back on the CPU."""
    assert buf.numel() == n + 2 * guard
    assert bool((buf[:guard] == SENTINEL).all()), (what, "bytes in front of the buffer were written")
    assert bool((buf[guard + n:] == SENTINEL).all()), (what, "bytes behind the buffer were written")


def bf16_from_bits(bits):
    """int tensor of 16-bit patterns -> bfloat16"""
    v = bits.to(torch.int64) << 16
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32).view(torch.float32).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ 1. quant_mxfp8: the value sweep
SWEEP_MANTISSAS = (0x00, 0x60, 0x61, 0x7F)                  # 1.0, exactly 1.75 (no step up), the first that steps up, the largest
SWEEP_EXTRA = (0x0000, 0x0001, 0x0040, 0x007F, 0x0020, 0x007E, 0x0000, 0x0002)    # +-0 and bf16 subnormals, in every block family
SWEEP_BLOCKS_PER_MAX = 67                                   # 16 * 128 swept magnitudes + extras over 31 free slots per block


@functools.lru_cache(maxsize=None)
def sweep():
    """-> (x bf16 [npix, 32], q, s): one block per pixel.  Maxima: every biased exponent 0..254 x SWEEP_MANTISSAS x both signs;
    the other 31 elements of a maximum's 67 blocks sweep all 128 mantissas at the 16 exponents from the maximum's down to 15 below
    (clipped to the maximum's magnitude; exponents below zero give +-0, exponent field 0 the bf16 subnormals) plus SWEEP_EXTRA.
    Element signs alternate irregularly and flip with the maximum's sign, so every magnitude occurs with both signs.  The maximum
    sits at a different channel of each block."""
    e = torch.arange(255).repeat_interleave(len(SWEEP_MANTISSAS))
    m = torch.tensor(SWEEP_MANTISSAS).repeat(255)
    maxmag = torch.cat([(e << 7) | m] * 2)                                              # [2040]
    maxsign = torch.cat([torch.zeros(e.numel(), dtype=torch.int64), torch.ones(e.numel(), dtype=torch.int64)])
    ee = torch.cat([e, e])[:, None, None] - torch.arange(16)[None, :, None]               # [2040, 16, 1]
    mag = torch.where(ee >= 0, (ee << 7) | torch.arange(128)[None, None, :], torch.zeros(1, dtype=torch.int64)).reshape(-1, 2048)
    n_free = SWEEP_BLOCKS_PER_MAX * 31
    extra = torch.tensor(SWEEP_EXTRA).repeat(-(-(n_free - 2048) // len(SWEEP_EXTRA)))[: n_free - 2048]
    mag = torch.cat([mag, extra[None, :].expand(mag.shape[0], -1)], 1)
    mag = torch.minimum(mag, maxmag[:, None])                                            # bit patterns order like magnitudes
    j = torch.arange(n_free)
    sign = ((((j * 0x9E37) >> 5) ^ j ^ (j >> 3)) & 1)[None, :] ^ maxsign[:, None]
    others = (mag | (sign << 15)).reshape(-1, 31)                                        # [2040 * 67, 31]
    nblk = others.shape[0]
    pos = (torch.arange(nblk) * 7 + 3) % 32
    bits = torch.zeros(nblk, 32, dtype=torch.int64)
    bits.scatter_(1, (pos[:, None] + 1 + torch.arange(31)[None, :]) % 32, others)
    bits.scatter_(1, pos[:, None], ((maxmag | (maxsign << 15)).repeat_interleave(SWEEP_BLOCKS_PER_MAX))[:, None])
    x = bf16_from_bits(bits)
    q, s, _ = MX.quantize(x.float())
    return x, q, s


def tie_counts(x, q, s):
    """(ties rounded down, ties rounded up) among the expected bytes: elements whose scaled value lies exactly half way between
    two neighbouring e4m3 code points (the other neighbour 2 * scaled - deq is a code point too)."""
    scaled = x.double().reshape(-1, 32) * torch.ldexp(torch.ones(s.numel(), dtype=torch.float64), 127 - s.reshape(-1).to(torch.int64))[:, None]
    deq = decode_e4m3(q).double().reshape(-1, 32)
    other = 2 * scaled - deq
    ok = torch.isfinite(scaled) & (scaled.abs() < 448) & (other != deq) & (other.abs() <= 448)
    rep = decode_e4m3(encode_e4m3(torch.where(ok, other, torch.zeros_like(other)))).double() == other
    tie = ok & rep
    up = deq.abs() > scaled.abs()
    return int((tie & ~up).sum()), int((tie & up).sum())


@functools.lru_cache(maxsize=None)
def nonfinite():
    """-> (x bf16 [64, 32], q, s): blocks whose maximum is +Inf / -Inf (scale byte 247, the infinity saturates to +-448, finite
    elements scale by 2^-120), NaNs beside finite elements (byte 0x7f; the block's scale comes from the finite elements), and a
    NaN and an infinity in one block."""
    g = torch.Generator().manual_seed(41)
    x = torch.randn(64, 32, generator=g) * torch.exp(12 * torch.randn(64, 1, generator=g))
    x[40:, :] = torch.randn(24, 32, generator=g) * 2.0 ** torch.randint(90, 127, (24, 1), generator=g).float()
    x = x.to(torch.bfloat16)
    for p in range(0, 64, 4):
        x[p, (p * 5) % 32] = float("inf")
        x[p + 1, (p * 3 + 1) % 32] = float("-inf")
        x[p + 2, (p * 7 + 2) % 32] = float("nan")
    x[3, 0], x[3, 31] = float("nan"), float("inf")
    x[7, 4], x[7, 5] = float("nan"), float("-inf")
    x[63, :] = bf16_from_bits(torch.tensor([0x7F7F, 0xFF7F] * 16))             # the largest finite bf16 beside an infinity
    x[63, 9] = float("inf")
    q, s, _ = MX.quantize(x.float())
    return x, q, s


# ------------------------------------------------------------------------------------------------ 1. quant_mxfp8: launch shapes
@dataclass(frozen=True)
class Launch:
    B: int                # grid rows ("samples")
    vpp: int              # 16-byte vectors per pixel
    pow2: bool
    hoist: bool           # GroupNorm variant only: coefficients loaded once per thread
    n: int                # vectors per sample
    stride: int           # grid stride in vectors
    trips: frozenset      # {(four-vector trips, single trips)} over the threads that do any work


def _launch(B, per, C, gn):
    vps = per * (C // 8)
    gx = max(1, min((vps + 255) // 256, (256 * 64 + B - 1) // B))
    stride = gx * 256
    vpp = C // 8
    pow2 = vpp & (vpp - 1) == 0
    counts = {-(-(vps - i0) // stride) for i0 in (0, min(vps, stride) - 1, (vps - 1) % stride, min((vps - 1) % stride + 1, min(vps, stride) - 1))}
    return Launch(B, vpp, pow2, bool(gn and pow2 and vpp <= 256), vps, stride, frozenset((k // 4, k % 4) for k in counts if k > 0))


def quant_launch(npix, C):
    """The launch quant_mxfp8() (quant_mxfp8.hip) makes for [npix][C]: its split into equal "samples" and the trip counts."""
    B, per = 1, npix
    for d in (4096, 1024, 256, 64, 16, 4, 2):
        if npix % d == 0 and npix // d >= 1024:
            B, per = d, npix // d
            break
    return _launch(B, per, C, False)


def gn_launch(B, hw, C):
    return _launch(B, hw, C, True)


# (npix, C): B = 1, 2 and 4096; C / 8 in {4, 12, 16, 48, 128, 192}; threads with one, two and three single trips behind a
# four-vector trip.  A thread makes more than one trip only when the tensor holds more than 256 * 64 * 256 vectors = 2^25 elements,
# and four only from 2^27 elements on, whatever the split - hence the three large shapes (data tiled from LAUNCH_PERIOD pixels).
LAUNCH_SHAPES = ((1000, 96), (2052, 128), (2048, 384), (64, 1024), (1030, 1536), (4096 * 1024, 32), (4096 * 1400, 32), (4096 * 1700, 32))
LAUNCH_PERIOD = 1021                                        # prime: no sample, block or grid-stride boundary repeats in the data


@functools.lru_cache(maxsize=None)
def launch_case(npix, C):
    """-> (base bf16 [P, C], q, s, P): pixel p of the tensor is base[p % P]; P = npix for the small shapes."""
    P = npix if npix * C <= (1 << 22) else LAUNCH_PERIOD
    g = torch.Generator().manual_seed(1000 + C + npix % 997)
    x = torch.randn(P, C, generator=g) * torch.exp(3 * torch.randn(P, 1, generator=g)) * torch.exp(2 * torch.randn(1, C // 32, generator=g)).repeat_interleave(32, 1)
    x[5] = 0
    x[6, :32] = 1e-30
    x[7, :32] = torch.tensor([2.0 ** (k % 9 - 4) for k in range(32)])
    x[8, -32:] = 1.75 * 2.0 ** 3                            # exactly on the boundary: no step up
    x[9, -32:] = 1.7578125 * 2.0 ** 3                       # one bf16 step above it
    x[10] = -0.0
    x[11, :32] = 3.0e38
    x = x.to(torch.bfloat16)
    x[12, :32] = bf16_from_bits(torch.arange(32) * 4 + 1)   # bf16 subnormals only
    x[P - 1, -32:] = bf16_from_bits(torch.arange(32) + 0x3F80 + 0x60 - 16)     # mantissas around 1.75 in the very last block
    q, s, _ = MX.quantize(x.float())
    return x, q, s, P


# ------------------------------------------------------------------------------------------------ 2. gn_apply_silu_mxfp8
GN_SHAPES = ((3, 256, 128), (3, 264, 128), (3, 256, 1024), (3, 264, 1024), (2, 264, 96), (2, 264, 384))     # (B, hw, C)
SILU_ID_MIN, SILU_ZERO_MAX = 32, -110     # t >= 32: 1 + exp(-t) == 1 in fp32, silu(t) = t; t <= -110: exp(-t) = inf, silu(t) = -0


@dataclass
class GnCase:
    x: torch.Tensor                        # bf16 [B, hw, C]
    a: torch.Tensor                        # fp32 [B, C]
    b: torch.Tensor
    q: torch.Tensor                        # expected
    s: torch.Tensor
    t: torch.Tensor = None                 # float64 a * x + b
    y: torch.Tensor = None                 # float64 silu(t)
    block_decided: torch.Tensor = None     # gaussian family only
    elem_decided: torch.Tensor = None


def _hash(*idx):
    h = torch.zeros((), dtype=torch.int64)
    for k, v in zip((7919, 104729, 1299709), idx):
        h = h + v.to(torch.int64) * k
    h = (h * 2654435761) & 0xFFFFFFFF
    return (h ^ (h >> 15)) & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def gn_exact(B, hw, C):
    """The `exact` family: a[b][c] = 2^(1 + (c + b) % 4), b[b][c] = a * ((3 c + 5 b) % 17 - 8) - distinct (a, b) pairs within a
    vector, between the four lanes of a block and between samples - and integer x with t = a * x + b either 32 * j (silu = t) or
    -256 (silu = -0).  Block (pixel p, block k) has scale exponent 7 or 8 in a checkerboard and its maximum 1.5 * 2^7 or 1.5 * 2^8
    at channel (7 p + 3 k + b) % 32; every t is 32 * j with j <= 6 or 12, so every scaled element is a multiple of 32 (64) up to 384:
    e4m3 code points, at the centre of their rounding intervals.  A relative error of 2^-23 in t * rcp(1) moves no byte."""
    sb_, p_, c_ = torch.arange(B)[:, None, None], torch.arange(hw)[None, :, None], torch.arange(C)[None, None, :]
    a = 2.0 ** (1 + (c_ + sb_) % 4).double()
    m = ((3 * c_ + 5 * sb_) % 17 - 8).double()
    blk = c_ // 32
    jmax = 6 * (1 + ((p_ + blk + sb_) & 1))
    h = _hash(sb_, p_, c_)
    j = 1 + h % jmax
    is_max = (c_ % 32) == (7 * p_ + 3 * blk + sb_) % 32
    j = torch.where(is_max, jmax, j)
    t = torch.where(((h >> 8) % 8 == 0) & ~is_max, torch.full_like(j, -256), 32 * j).double()
    x = t / a - m
    y = torch.where(t >= SILU_ID_MIN, t, torch.full_like(t, -0.0))
    q, s, _ = MX.quantize(y.float())
    return GnCase(x.to(torch.bfloat16), a[:, 0, :].float().contiguous(), (a * m)[:, 0, :].float().contiguous(), q, s, t, y)


def silu64(t):
    return t / (1 + torch.exp(-t))


def gn_delta(t):
    """Relative error bound of the device's y = t * rcp(1 + exp2(-t * log2 e)) against silu64(t): v_exp_f32 and v_rcp_f32 at
    1 ulp each, the rounding of t * log2 e (|t| * 2^-24 relative in the exponential), the roundings of a * x + b, of 1 + e and of
    the final product (common.hpp, silu<false>): (|t| + 8) * 2^-24."""
    return (t.abs() + 8) * 2.0 ** -24


def gn_reference(x, a, b, *, coef_vector_shift=0, sample0_coefs=False, round_y_to_bf16=False):
    """float64 silu(a x + b) -> (q, s, t, y); the keyword arguments are the mutants of section 2."""
    if coef_vector_shift:
        a, b = torch.roll(a, -8 * coef_vector_shift, 1), torch.roll(b, -8 * coef_vector_shift, 1)
    if sample0_coefs:
        a, b = a[:1].expand_as(a), b[:1].expand_as(b)
    t = a.double()[:, None, :] * x.double() + b.double()[:, None, :]
    y = silu64(t)
    y32 = y.float()
    if round_y_to_bf16:
        y32 = y32.to(torch.bfloat16).float()
    q, s, _ = MX.quantize(y32)
    return q, s, t, y


@functools.lru_cache(maxsize=None)
def gn_gaussian(B, hw, C):
    """The `gaussian` family: x ~ 2 N(0, 1) in bf16, a ~ 1 + 0.3 N, b ~ 0.5 N (what a ResnetBlock feeds the kernel); expected bytes
    = MX.quantize(float32(silu64(a x + b))).  A block is decided when its scale byte is the same for |y| (1 - delta) and
    |y| (1 + delta), an element when its block is and its byte is the same at both ends (gn_delta)."""
    g = torch.Generator().manual_seed(7000 + 13 * C + hw)
    x = (2 * torch.randn(B, hw, C, generator=g)).to(torch.bfloat16)
    a = (1 + 0.3 * torch.randn(B, C, generator=g)).float()
    b = (0.5 * torch.randn(B, C, generator=g)).float()
    q, s, t, y = gn_reference(x, a, b)
    d = gn_delta(t)
    lo, hi = y * (1 - d), y * (1 + d)
    s_lo = scale_byte(lo.abs().reshape(B, hw, C // 32, 32).amax(-1))
    s_hi = scale_byte(hi.abs().reshape(B, hw, C // 32, 32).amax(-1))
    block_decided = (s_lo == s) & (s_hi == s)
    inv = torch.ldexp(torch.ones(s.shape, dtype=torch.float64), 127 - s.to(torch.int64)).repeat_interleave(32, -1)
    q_lo, q_hi = encode_e4m3(lo * inv), encode_e4m3(hi * inv)
    elem_decided = block_decided.repeat_interleave(32, -1) & (q_lo == q) & (q_hi == q)
    return GnCase(x, a, b, q, s, t, y, block_decided, elem_decided)


UNDECIDED_CAP = 1e-3                                        # share of undecided blocks / elements the gaussian data may have


def undecided_shares(case):
    return 1 - float(case.block_decided.double().mean()), 1 - float(case.elem_decided.double().mean())


def assert_gn_gaussian(got_q, got_s, case, what=""):
    """Decided blocks and elements bit-equal; undecided elements within one e4m3 code step of the expected value."""
    want_q, want_s = case.q, case.s
    got_q, got_s = got_q.reshape(want_q.shape), got_s.reshape(want_s.shape)
    bd, ed = case.block_decided, case.elem_decided
    bad = (bd & (got_s != want_s)).nonzero()
    assert bad.numel() == 0, (what, "scale byte of a decided block", int(bad.shape[0]), bad[:4].tolist())
    bad = (ed & (got_q != want_q)).nonzero()
    assert bad.numel() == 0, (what, "byte of a decided element", int(bad.shape[0]), bad[:4].tolist(),
                              hex(int(got_q[tuple(bad[0])])), hex(int(want_q[tuple(bad[0])])))
    ds = (got_s.to(torch.int32) - want_s.to(torch.int32)).abs()
    assert int(ds.max()) <= 1, (what, "scale byte of an undecided block off by more than one")
    # undecided elements of a decided block: neighbouring codes (+0 and -0 are one value)
    bdx = bd.repeat_interleave(32, -1)
    und = ~ed & bdx
    gm, wm = (got_q & 0x7F).to(torch.int32), (want_q & 0x7F).to(torch.int32)
    same_sign = ((got_q ^ want_q) & 0x80) == 0
    near = (same_sign & ((gm - wm).abs() <= 1)) | (~same_sign & (gm + wm <= 1))
    bad = (und & ~near).nonzero()
    assert bad.numel() == 0, (what, "undecided element more than one code step away", int(bad.shape[0]), bad[:4].tolist())
    # elements of an undecided block: one step of the coarser of the two scales
    unb = ~bdx
    if bool(unb.any()):
        sc_g = torch.ldexp(torch.ones(got_s.shape, dtype=torch.float64), got_s.to(torch.int64) - 127).repeat_interleave(32, -1)
        sc_w = torch.ldexp(torch.ones(want_s.shape, dtype=torch.float64), want_s.to(torch.int64) - 127).repeat_interleave(32, -1)
        dg, dw = decode_e4m3(got_q).double() * sc_g, decode_e4m3(want_q).double() * sc_w
        step = torch.maximum(dw.abs() * 2.0 ** -3, torch.maximum(sc_g, sc_w) * 2.0 ** -9)
        bad = (unb & ~((dg - dw).abs() <= step)).nonzero()
        assert bad.numel() == 0, (what, "element of an undecided block more than one step away", int(bad.shape[0]), bad[:4].tolist())


# ------------------------------------------------------------------------------------------------ 3. the fused twins
def channel_exponent(o):
    return (o // 32 * 5 + o // 128 * 3) % 11 - 5


def pixel_exponent(p):
    return p % 7 - 3


def ramp_exponent(H, W):
    """[H, W] input exponents for the sites whose output pixel reads a WINDOW of input pixels (the 3x3 convolutions, the
    input-convolution form).  p mod 7 cannot work there: at W = 32 every 3x3 window holds all seven residues, so every output
    pixel would see the same largest input scale.  On the ramp x + y the largest scale inside a window is that of its last
    pixel, which differs between any two neighbouring windows."""
    return torch.arange(H)[:, None] + torch.arange(W)[None, :] - (H + W) // 2


def assert_scale_diversity(s, what=""):
    """s [B, H, W, nblk] expected scale bytes: at least 90 % of horizontally adjacent block pairs (same pixel) and at least 50 % of
    adjacent pixel pairs (same block, along W) differ - else a scale byte written for the wrong block would not show."""
    blocks = float((s[..., 1:] != s[..., :-1]).double().mean())
    pixels = float((s[:, :, 1:, :] != s[:, :, :-1, :]).double().mean())
    assert blocks >= 0.9 and pixels >= 0.5, (what, blocks, pixels)
    return blocks, pixels


def assert_stored_blockwise(got_nhwc, want_nhwc, what=""):
    """The stored tensor of a site WITHOUT an additive epilogue, block by block: within every 32-channel block of a pixel the
    largest error is at most 2^-7 of the block's largest reference value.  The bf16 store (8 significant bits) costs up to 2^-8
    of an element, hence of the block's maximum; as much again is allowed for the fp32 summation order of the kernel and of the
    reference, which is about sqrt(K) * 2^-24 of an element and has no useful worst-case bound (measured on MI355X: 0.0038 - 0.0039
    = the store alone).  The parity tolerances of tests/test_kernels_gpu.py are relative to the TENSOR's maximum, and these
    tensors span 2^20 and more: without this a twin of noise in the small blocks would pass."""
    g = got_nhwc.float().reshape(-1, 32)
    w = want_nhwc.float().reshape(-1, 32)
    err, ref = (g - w).abs().amax(1), w.abs().amax(1)
    ratio = float((err / ref.clamp(min=1e-30)).max())
    assert bool((err <= ref * 2.0 ** -7).all()), (what, ratio)
    return ratio


def assert_twin(q, s, stored, what=""):
    """The definition of a twin: MX.quantize of the bf16 tensor the same call stored.  stored: [..., C] bf16 / float."""
    want_q, want_s, _ = MX.quantize(stored.float())
    assert_bytes(q, s, want_q, want_s, what)


@dataclass
class TwinConv:
    name: str
    impl: int                              # 3 = conv1x1_bf16, 4 = conv1x1_mxfp8, 0 = conv3x3_mxfp8 (its own entry point)
    x0: torch.Tensor                       # NCHW fp32, bf16-exact
    x1: torch.Tensor
    w: torch.Tensor                        # OIHW fp32 (impl 3: bf16-exact)
    b: torch.Tensor
    kw: dict                               # ks / stride / pad / kind of run_conv
    residual: torch.Tensor = None
    gn_tail: tuple = None                  # (h, a, b)
    groups: int = 0
    window: tuple = None                   # (ps0, Wout): the input-convolution form; x0 is then [B, Hin, Win, ps0] NHWC
    want: torch.Tensor = None              # NCHW fp32: the stored tensor's reference (before the bf16 store)
    out_shape: tuple = None                # NHWC shape of the stored tensor


def _bf(t):
    return t.to(torch.bfloat16).float()


def _scaled_input(g, B, C, H, W, ramp=False):
    x = torch.randn(B, C, H, W, generator=g)
    e = ramp_exponent(H, W) if ramp else pixel_exponent(torch.arange(H * W).reshape(H, W))
    return _bf(x * 2.0 ** e.float())


def _row_scale(cout):
    return 2.0 ** channel_exponent(torch.arange(cout)).float()


def _mx_deq(x_nchw):
    _, _, deq = MX.quantize(x_nchw.permute(0, 2, 3, 1).contiguous())
    return deq.permute(0, 3, 1, 2)


def mx_pointwise_reference(x0, x1, w_oi, b, taps=1):
    """conv1x1_mxfp8's arithmetic (tests/test_kernels_gpu.py, _mx_pointwise_reference): MX-quantised sources and weights, exact
    products; taps = 4: the 2x2 / stride-2 gather, tap-major weights."""
    xq = torch.cat([_mx_deq(t) for t in (x0, x1) if t is not None], 1)
    if taps == 1:
        _, _, wq = MX.quantize(w_oi.reshape(w_oi.shape[0], -1))
        return F.conv2d(xq.double(), wq.reshape(*w_oi.shape[:2], 1, 1).double(), b.double()).float()
    cout, c4 = w_oi.shape[:2]
    w4 = w_oi.reshape(cout, c4 // 4, 2, 2).permute(0, 2, 3, 1).contiguous()
    _, _, w4q = MX.quantize(w4)
    return F.conv2d(xq.double(), w4q.permute(0, 3, 1, 2).double(), b.double(), stride=2).float()


def mx_conv3x3_reference(x0, x1, w, b):
    xq = torch.cat([_mx_deq(t) for t in (x0, x1) if t is not None], 1)
    return F.conv2d(xq.double(), MX.quantize_conv_weight(w).double(), b.double(), padding=1).float()


TWIN_VARIANTS_BF16 = ("plain", "residual", "gn_tail", "pixel_shuffle", "unshuffle", "input_conv")
TWIN_VARIANTS_MX = ("plain", "residual", "gn_tail", "pixel_shuffle", "unshuffle")
TWIN_3X3 = (("c128", 2, 128, 0, 128, 8, 32), ("c128_256", 2, 128, 256, 256, 16, 32))       # name, B, C0, C1, Cout, H, W


@functools.lru_cache(maxsize=None)
def twin_conv_case(impl, variant):
    """The pointwise sites: conv1x1_bf16 (impl 3) and conv1x1_mxfp8 (impl 4).  Weight rows of output channel o carry
    2^channel_exponent(o), the input of pixel p 2^pixel_exponent(p) (the input-convolution form: ramp_exponent): neighbouring
    blocks and pixels get different scale bytes."""
    g = torch.Generator().manual_seed(300 + impl * 10 + TWIN_VARIANTS_BF16.index(variant))
    B, H, W = 2, 16, 32
    mx = impl == 4
    rw = (lambda t: t) if mx else _bf
    kw = dict(ks=1, stride=1, pad=0, kind=0)
    c = TwinConv(variant, impl, None, None, None, None, kw)
    if variant == "pixel_shuffle":
        c.x0 = _scaled_input(g, B, 128, H, W)
        # the twin's channel of convolution row o is o // 4 (the other two bits select the pixel of the 2x2 cell)
        rs = _row_scale(128).repeat_interleave(4)
        c.w = rw(torch.randn(512, 128, 1, 1, generator=g) / 11 * rs[:, None, None, None])
        c.b = torch.randn(512, generator=g) * rs * 0.1
        kw["kind"] = 2
        pre = mx_pointwise_reference(c.x0, None, c.w[:, :, 0, 0], c.b) if mx else F.conv2d(c.x0, c.w, c.b)
        c.want = F.pixel_shuffle(F.silu(pre), 2)
    elif variant == "unshuffle":
        c.x0 = _scaled_input(g, B, 128, 2 * H, 2 * W)
        c.w = rw(torch.randn(128, 512, 1, 1, generator=g) / 22 * _row_scale(128)[:, None, None, None])
        c.b = torch.randn(128, generator=g) * _row_scale(128) * 0.1
        kw.update(ks=2, stride=2, kind=1)
        if mx:
            c.want = mx_pointwise_reference(c.x0, None, c.w[:, :, 0, 0], c.b, taps=4)
        else:
            c.want = F.conv2d(F.pixel_unshuffle(c.x0, 2), c.w, c.b)
    elif variant == "input_conv":
        # the 7x7 input convolution as the engine runs it: [B][H + 6][W + 8][8] gathered image, a 7x1 kernel over 64 "channels"
        # (8 pixels x 8 channels) whose pixels lie 8 elements apart.  Output pixel (y, x) reads elements 8 x .. 8 x + 63 of rows y .. y + 6.
        assert not mx
        Hin, Win = H + 6, W + 8
        img = torch.randn(B, Hin, Win, 8, generator=g)
        img = _bf(img * 2.0 ** ramp_exponent(Hin, Win).float()[None, :, :, None])
        c.x0 = img
        c.w = _bf(torch.randn(128, 64, 7, 1, generator=g) / 21 * _row_scale(128)[:, None, None, None])
        c.b = torch.randn(128, generator=g) * _row_scale(128) * 0.1
        kw.update(ks=7)
        c.window = (8, W)
        flat = img.reshape(B, Hin, Win * 8)
        cols = torch.stack([flat[:, :, 8 * x: 8 * x + 64] for x in range(W)], 2)            # [B, Hin, W, 64]
        rows = torch.stack([cols[:, dy: dy + H] for dy in range(7)], -1)                     # [B, H, W, 64, 7]
        c.want = (torch.einsum("bhwcd,ocd->bohw", rows.double(), c.w[:, :, :, 0].double()) + c.b.double()[None, :, None, None]).float()
    else:
        c.x0, c.x1 = _scaled_input(g, B, 128, H, W), _scaled_input(g, B, 128, H, W)
        c.w = rw(torch.randn(128, 256, 1, 1, generator=g) / 16 * _row_scale(128)[:, None, None, None])
        c.b = torch.randn(128, generator=g) * _row_scale(128) * 0.1
        want = mx_pointwise_reference(c.x0, c.x1, c.w[:, :, 0, 0], c.b) if mx else F.conv2d(torch.cat((c.x0, c.x1), 1), c.w, c.b)
        if variant == "residual":
            c.residual = _bf(torch.randn(B, 128, H, W, generator=g) * 0.5 * _row_scale(128)[None, :, None, None]
                             * 2.0 ** pixel_exponent(torch.arange(H * W).reshape(1, 1, H, W)).float())
            want = (_bf(want) if mx else want) + c.residual
        if variant == "gn_tail":
            h = _scaled_input(g, B, 128, H, W)
            ca = (1 + 0.3 * torch.randn(B, 128, generator=g)) * _row_scale(128)
            cb = 0.5 * torch.randn(B, 128, generator=g) * _row_scale(128)
            c.gn_tail = (h, ca, cb)
            want = F.silu(ca[:, :, None, None] * h + cb[:, :, None, None]) + (_bf(want) if mx else want)
        c.want = want
    c.out_shape = (c.want.shape[0], c.want.shape[2], c.want.shape[3], c.want.shape[1])
    return c


@functools.lru_cache(maxsize=None)
def twin_conv3x3_case(name):
    _, B, C0, C1, Cout, H, W = next(t for t in TWIN_3X3 if t[0] == name)
    g = torch.Generator().manual_seed(400 + C1)
    x0 = _scaled_input(g, B, C0, H, W, ramp=True)
    x1 = _scaled_input(g, B, C1, H, W, ramp=True) if C1 else None
    w = torch.randn(Cout, C0 + C1, 3, 3, generator=g) / (9 * (C0 + C1)) ** 0.5 * _row_scale(Cout)[:, None, None, None]
    b = 0.1 * torch.randn(Cout, generator=g) * _row_scale(Cout)
    c = TwinConv(name, 0, x0, x1, w, b, dict(ks=3, stride=1, pad=1, kind=0), groups=8)
    c.want = mx_conv3x3_reference(x0, x1, w, b)
    c.out_shape = (B, H, W, Cout)
    return c


def stored_nhwc(want_nchw):
    """The CPU stand-in for the stored tensor: the reference rounded to bf16, NHWC."""
    return want_nchw.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def unshuffled_twin(pre_nchw):
    """Mutant of the PixelShuffle twin: the bytes of the [B, H, W, Cout] tensor before the shuffle, read as [B, 2H, 2W, Cout / 4]."""
    q, s, _ = MX.quantize(stored_nhwc(pre_nchw).float())
    return q.reshape(-1), s.reshape(-1)


TWIN_GN = ((3, 264, 128), (3, 264, 384))                    # (B, hw, C): HOIST and non-HOIST of gn_apply_kernel


@dataclass
class TwinGn:
    x: torch.Tensor                        # bf16 [B, hw, C]
    residual: torch.Tensor                 # bf16 [B, hw, C] or None
    gamma: torch.Tensor
    beta: torch.Tensor
    partial: torch.Tensor                  # fp32 [B, groups, 1, 2]: (sum, sum of squares) of x per (sample, group), one slot
    groups: int
    want: torch.Tensor                     # fp32 [B, hw, C]


@functools.lru_cache(maxsize=None)
def twin_gn_case(B, hw, C, with_residual):
    """gn_apply_silu with its twin, through srgd_k_groupnorm_silu_twin: gamma of channel c carries 2^channel_exponent(c); the
    input's spread at pixel p is 2^pixel_exponent(p) (GroupNorm normalises over the whole image, so the spread survives it), and the
    residual, where there is one, carries both factors."""
    groups = 8
    g = torch.Generator().manual_seed(500 + C + int(with_residual))
    p = torch.arange(hw)[None, :, None]
    x = (torch.randn(B, hw, C, generator=g) * 2.0 ** pixel_exponent(p).float() + 0.3).to(torch.bfloat16)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)) * _row_scale(C)
    beta = 0.3 * torch.randn(C, generator=g) * _row_scale(C)
    res = (torch.randn(B, hw, C, generator=g) * 2.0 ** pixel_exponent(p).float() * _row_scale(C)).to(torch.bfloat16) if with_residual else None
    xg = x.double().reshape(B, hw, groups, C // groups)
    partial = torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], -1).reshape(B, groups, 1, 2).float().contiguous()
    y = F.group_norm(x.float().permute(0, 2, 1), groups, gamma, beta, eps=1e-5).permute(0, 2, 1)
    want = F.silu(y) + (res.float() if with_residual else 0)
    return TwinGn(x, res, gamma.float(), beta.float(), partial, groups, want.contiguous())


# ------------------------------------------------------------------------------------------------ 4. host weight quantisers
def weight_blocks(n, seed):
    """n designed 32-element weight blocks, fp32 [n, 32]: maxima 1.75 * 2^k and one float above it over a wide exponent range,
    exact ties, elements in the e4m3 subnormal range of their block, all-zero blocks, random blocks.  Every value times the
    block's inverse scale is an fp32 normal; the dequantised weights are fp32 normals too (the fp32-subnormal block is
    `subnormal_block`)."""
    g = torch.Generator().manual_seed(seed)
    blk = torch.zeros(n, 32)
    one_up = torch.tensor(1.75).view(torch.int32).add(1).view(torch.float32).item()
    for i in range(n):
        kind = i % 6
        k = float((i * 7) % 61 - 30)
        if kind == 0:                                        # all zero
            continue
        if kind == 5:                                        # random
            blk[i] = torch.randn(32, generator=g) * 2.0 ** k
            continue
        top = {1: 1.75, 2: one_up, 3: 1.0, 4: 1.9990234375}[kind] * 2.0 ** k
        sc = 2.0 ** (k - 8 + (1 if kind in (2, 4) else 0))   # the block's scale under the engine's rule
        j = torch.arange(32)
        # exact ties between neighbouring code points (odd multiples of half a step) in the normal range, multiples and half
        # multiples of the subnormal step 2^-9, and plain random elements
        ties = (16 + 2 * (j % 8) + 1) / 16.0 * 2.0 ** (j % 4).float() * 8        # (2 m + 1) / 16 * 2^e: half way between mantissas
        sub = ((j // 3) % 16 + ((j // 3) % 4 == 1) * 0.5) * 2.0 ** -9            # odd multiples too: lost at any coarser scale
        rnd = torch.rand(32, generator=g) * 200
        v = torch.where(j % 3 == 0, ties, torch.where(j % 3 == 1, sub, rnd)) * sc
        v = v * torch.where(torch.rand(32, generator=g) < 0.5, -1.0, 1.0)
        v[(i * 5) % 32] = top * (-1.0 if i % 4 == 3 else 1.0)
        blk[i] = v
    return blk


def subnormal_block():
    """A block whose maximum is an fp32 subnormal: 1.5 * 2^-127; elements j * 2^-130 (scale byte 0: scaled by 2^127 they are
    j / 8 <= 1.5, code points, and the dequantised values are multiples of 2^-133, exact in bf16's subnormal range)."""
    v = torch.arange(32).double() % 13 * 2.0 ** -130
    v[5] = 1.5 * 2.0 ** -127
    v[6] = -v[6]
    return v.float()


def wrong_pow2_weight_quantizer(w_blocks):
    """Mutant of the host quantiser: floor(log2 amax) one too small at exact powers of two.  [.., 32] -> dequantised."""
    q, s = ref_quantize(w_blocks, log2="pow2_off")
    return decode_e4m3(q) * torch.ldexp(torch.ones(s.shape), s.to(torch.int32) - 127)[..., None].expand(*s.shape, 32).reshape(q.shape)


def dequantize_blocks(w_blocks):
    _, _, deq = MX.quantize(w_blocks)
    return deq


@functools.lru_cache(maxsize=None)
def weight_case(taps, Cin, Cout, seed, int_bias=False, with_subnormal=False):
    """-> (w [Cout, taps, Cin] fp32 (tap-major, blocks of 32 along Cin), bias [Cout], deq [Cout, taps, Cin])."""
    n = Cout * taps * Cin // 32
    blk = weight_blocks(n, seed)
    if with_subnormal:
        blk[7] = subnormal_block()
    w = blk.reshape(Cout, taps, Cin)
    bias = ((torch.arange(Cout) * 5) % 9 - 4).float() if int_bias else torch.zeros(Cout)
    return w, bias, dequantize_blocks(w)


def assert_weights_read_back(got, w_deq, bias, what=""):
    """got / w_deq: [Cout, taps, Cin] - what the one-hot convolution returned and deq(w); got == bf16(deq + bias) bit for bit
    (with a zero bias the sum IS deq: at most four significant bits, exact in bf16)."""
    want = (w_deq.double() + bias.double()[:, None, None]).float()
    if not bool((bias != 0).any()):
        assert torch.equal(want.to(torch.bfloat16).float(), want), "dequantised weights must be exact in bf16"
    want = want.to(torch.bfloat16).float()
    bad = (got != want).nonzero()                            # (+0 and -0 are one weight: the accumulator starts at +0)
    assert bad.numel() == 0, (what, int(bad.shape[0]), bad[:4].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


def onehot_3x3(Cin, H, W):
    """-> (x NCHW [B, Cin, H, W], sites [(b, y, x, c)]): ones on a stride-3 pixel grid (interior pixels, so that all nine taps
    land inside), a different channel at each.  Output (b, y - dy + 1, x - dx + 1, o) = deq(w[o, c, dy, dx]) + bias."""
    ys, xs = list(range(1, H - 1, 3)), list(range(1, W - 1, 3))
    per = len(ys) * len(xs)
    B = -(-Cin // per)
    x = torch.zeros(B, Cin, H, W)
    sites = []
    for c in range(Cin):
        b, r = divmod(c, per)
        y, xx = ys[r // len(xs)], xs[r % len(xs)]
        x[b, c, y, xx] = 1.0
        sites.append((b, y, xx, c))
    return x, sites


def read_back_3x3(out_nchw, sites, Cout):
    """-> [Cout, 9, Cin]: tap (dy, dx) of input channel c, read from the output pixel it alone reaches."""
    got = torch.zeros(Cout, 9, len(sites))
    for (b, y, x, c) in sites:
        for dy in range(3):
            for dx in range(3):
                got[:, dy * 3 + dx, c] = out_nchw[b, :, y - dy + 1, x - dx + 1]
    return got
