"""Inputs for the attention kernels whose exact output is known in closed form, plus the assertions that go with them.

Pure torch on the CPU; test infrastructure only (used by tests/test_attention_exact_gpu.py, which feeds the tensors to the HIP
kernels, and by tests/test_attention_cases_cpu.py, which proves the constructions against the float64 oracle and shows that the
assertions reject a subtly wrong attention).  Every tensor is the NCHW `qkv` of the model, [B, 3*heads*32, H, W] with channel
= part*heads*32 + head*32 + d and position n = y*W + x, and its expected output [B, heads*32, H, W].

Why closed forms: on Gaussian data one key out of 1024 dropped, doubled or paired with the wrong V row moves the output by
~1e-3 relative, ten times below the bf16 tolerance of the parity tests.  Here the softmax is forced to be exactly one-hot
(A, C: the output must be one V row, bit for bit - catches a wrong pairing, a lost key, a bad rescale) or exactly uniform
(B, D: the output is the plain sum of small integers over all keys - counts every key once).  The two kinds are both needed:
a key counted twice in numerator and denominator is invisible to A / C, two V rows swapped are invisible to B / D.
"""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

DH = 32                                   # dim_head of every attention site
LEAD = 110.0                              # exp(-110) = 2^-158.7: below half the smallest fp32 denormal, so exactly 0 in fp32
SCALE32 = float(np.float32(1.0) / np.sqrt(np.float32(DH)))      # what linear_attention() computes on the host: 1.0f / sqrtf(32)
CAP_FP32 = 2 ** 12                        # max |S_e| of a counting case run in fp32
CAP_BF16 = 64                             # ... with bf16 output: one key of weight >= 1 is >= 2^-6 = 4 x the 2^-8 tolerance
REL_FP32 = 2.0 ** -21                     # one reciprocal (<= 2.5 ulp if the compiler's fast form is used) + one multiply, doubled
REL_BF16 = 2.0 ** -8                      # one output rounding (2^-9), doubled


@dataclass
class Case:
    qkv: torch.Tensor                     # [B, 3*heads*32, H, W] fp32, every value exact in bf16
    want: torch.Tensor                    # [B, heads*32, H, W]; fp32 when `exact`, float64 otherwise
    exact: bool                           # True: bit-equal (after bf16 rounding of `want` in bf16 mode); False: REL_* relative
    heads: int
    meta: dict = field(default_factory=dict)


def hw_of(n):
    """Any H x W = n (the kernels only see n): the most square factorisation."""
    h = max(d for d in range(1, math.isqrt(n) + 1) if n % d == 0)
    return h, n // h


def bf16_round(x):
    return x.to(torch.bfloat16).float()


def _pack(q, k, v):
    """q, k, v [B, heads, 32, n] -> qkv [B, 3*heads*32, H, W]."""
    b, heads, _, n = q.shape
    return torch.stack((q, k, v), 1).reshape(b, 3 * heads * DH, *hw_of(n)).contiguous()


def _nchw(out):
    b, heads, _, n = out.shape
    return out.reshape(b, heads * DH, *hw_of(n)).contiguous()


# ---------------------------------------------------------------------------------------------- A: full attention, permutation
def permutation_code(n):
    """(bits, reps, a): key j carries the +-1 binary index of j, `bits` wide, repeated `reps` times and padded with +1 to 32
    entries, so two codes differ in >= reps places and the matching key leads every other logit by 2*reps*a/sqrt(32);
    a = the smallest power of two that makes this lead >= LEAD."""
    bits = max(1, (n - 1).bit_length())
    reps = DH // bits
    a = 1.0
    while 2 * reps * a / math.sqrt(DH) < LEAD:
        a *= 2
    return bits, reps, a


def key_codes(n):
    bits, reps, _ = permutation_code(n)
    j = torch.arange(n)
    b = (((j[:, None] >> torch.arange(bits)) & 1) * 2 - 1).float()
    u = torch.ones(n, DH)
    u[:, :bits * reps] = b.repeat(1, reps)
    return u                                                               # [n, 32]


def full_permutation(B, heads, n, seed=0):
    """A.  k_j = u_j, q_i = a * u_pi(i) with a random permutation pi per (sample, head): softmax row i is exactly one-hot at
    pi(i) in fp32 (every other exp underflows to 0, l = 1), so out[i] = v[pi(i)] bit for bit, in fp32 and in bf16 mode.  Logits
    reach 32*a/sqrt(32) (724; 1448 at n = 4096), and wherever pi(i) lies in a late key block everything accumulated before it
    must be rescaled by exp(m - mn) = 0."""
    g = torch.Generator().manual_seed(1000 + seed)
    _, _, a = permutation_code(n)
    u = key_codes(n)
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(B * heads)]).reshape(B, heads, n)
    k = u.t().expand(B, heads, DH, n)
    q = (a * u[perm]).transpose(2, 3)                                      # [B, heads, 32, n]
    v = bf16_round(torch.randn(B, heads, DH, n, generator=g) * 2)
    want = torch.gather(v, 3, perm[:, :, None, :].expand(-1, -1, DH, -1))
    return Case(_pack(q, k, v), _nchw(want), True, heads, {"perm": perm, "max_logit": DH * a / math.sqrt(DH)})


# ---------------------------------------------------------------------------------------------- B / D: counting values
def counting_weights(n, cap):
    """Integer weight per key / position for the counting cases, 0 = not covered, the densest of three layouts whose channel
    sums stay <= cap (the i-th covered key goes to channel i % 32, so a channel sums every 32nd covered key):
      "w123"   every key, weight 1 + (j // 32) % 3: distinct keys of a channel carry different weights
      "ones"   every key, weight 1 (n <= 32 * cap)
      "sparse" weight 1 on at most 32 * cap keys: the first and last 16, the four keys around every multiple of 512 (the chunk
               seams of linear attention: s-2, s-1, s, s+1), and one key in every `stride` with a phase that walks through all
               residues (j = i*stride + 7*i % stride); every other key carries v = 0 and such a case does not count it.
    Returns (weights [n] int64, layout name)."""
    j = torch.arange(n)
    w = 1 + (j // 32) % 3
    if int(channel_sums(w).max()) <= cap:
        return w, "w123"
    if (n + 31) // 32 <= cap:
        return torch.ones(n, dtype=torch.int64), "ones"
    must = set(range(16)) | set(range(n - 16, n))
    for s in range(512, n, 512):
        must |= {s - 2, s - 1, s, s + 1}
    stride = -(-n // (32 * cap - len(must)))
    picks = {i * stride + (7 * i) % stride for i in range(n // stride)}
    w = torch.zeros(n, dtype=torch.int64)
    w[sorted(must | picks)] = 1
    return w, "sparse"


def channel_sums(w):
    """[32] per-channel sums S_e of a weight vector under the 'i-th covered key -> channel i % 32' placement."""
    cov = w.nonzero().flatten()
    s = torch.zeros(DH, dtype=torch.int64)
    s.index_add_(0, torch.arange(cov.numel()) % DH, w[cov])
    return s


def _counting_v(B, heads, n, cap):
    """v [B, heads, 32, n] with key j's weight in one channel (rotated per sample and head so that a wrong head or sample stride
    lands on other sums), and S [B, heads, 32]."""
    w, layout = counting_weights(n, cap)
    cov = w.nonzero().flatten()
    rank = torch.arange(cov.numel())
    v = torch.zeros(B, heads, DH, n)
    for b in range(B):
        for h in range(heads):
            v[b, h, (rank + 5 * h + 11 * b) % DH, cov] = w[cov].float()
    S = v.double().sum(3)
    return v, S, {"layout": layout, "covered": cov, "smax": float(S.abs().max()), "cap": cap}


def full_uniform(B, heads, n, cap, seed=0):
    """B.  q = 0: every logit is 0, every p = 1 exactly, l = n, out[i, e] = S_e / n with S_e = sum_j v[j, e] - counts every
    covered key exactly once.  A power-of-two n is bit-exact (S_e and 1/n are exact), any other n within REL_*."""
    g = torch.Generator().manual_seed(2000 + seed)
    v, S, meta = _counting_v(B, heads, n, cap)
    k = bf16_round(torch.randn(B, heads, DH, n, generator=g))              # 0 * k = 0 whatever k holds
    q = torch.zeros(B, heads, DH, n)
    want = (S / n)[..., None].expand(-1, -1, -1, n)
    exact = n & (n - 1) == 0
    return Case(_pack(q, k, v), _nchw(want.float() if exact else want), exact, heads, meta)


# ---------------------------------------------------------------------------------------------- C: linear attention, selection
def seam_positions(n, limit):
    """Where chunked position handling can go wrong, most important first, at most `limit`: n = 0 and n - 1 (the last position
    of a ragged last chunk / of an odd n), then both sides of every multiple of 1024, then of every other multiple of 512."""
    out = [0, n - 1]
    for s in list(range(1024, n, 1024)) + list(range(512, n, 1024)):
        out += [s - 1, s]
    seen, uniq = set(), []
    for p in out:
        if 0 <= p < n and p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq[:limit]


def _one_hot_q(B, heads, n, g):
    dstar = torch.randint(0, DH, (B, heads, n), generator=g)
    q = torch.zeros(B, heads, DH, n)
    q.scatter_(2, dstar[:, :, None, :], 128.0)
    return q, dstar


def linear_selection(B, heads, n, seed=0):
    """C.  k[d, :] = 128 at one position p(d) and 0 elsewhere, q[:, n] = 128 at one channel d*(n): both softmaxes are exactly
    one-hot in fp32 (exp(-128) = 0), so ctx[d, e] = v[e, p(d)] and out[e, n] = fl32(v[e, p(d*(n))] * fl32(1/sqrt(32))), bit for
    bit (bf16 mode: its bf16 rounding).  A chunk without the spike must merge with weight exp(0 - 128) = 0.  The p(d) of the
    B*heads*32 (sample, head, d) slots take `seam_positions` first, scattered over the slots; the rest are random."""
    g = torch.Generator().manual_seed(3000 + seed)
    slots = B * heads * DH
    p = torch.randint(0, n, (slots,), generator=g)
    special = seam_positions(n, slots)
    p[torch.randperm(slots, generator=g)[:len(special)]] = torch.tensor(special)
    p = p.reshape(B, heads, DH)
    k = torch.zeros(B, heads, DH, n)
    k.scatter_(3, p[..., None], 128.0)
    q, dstar = _one_hot_q(B, heads, n, g)
    v = bf16_round(torch.randn(B, heads, DH, n, generator=g) * 2)
    pn = torch.gather(p, 2, dstar)                                         # [B, heads, n] = p(d*(n))
    want = torch.gather(v, 3, pn[:, :, None, :].expand(-1, -1, DH, -1)) * torch.tensor(SCALE32, dtype=torch.float32)
    return Case(_pack(q, k, v), _nchw(want), True, heads, {"p": p, "dstar": dstar, "special": special})


# ---------------------------------------------------------------------------------------------- D: linear attention, uniform
def linear_uniform(B, heads, n, cap, seed=0):
    """D.  k = 0: the position softmax is exactly uniform (p = 1, l = n), ctx[d, e] = S_e / n for every d; q one-hot as in C:
    out[e, n] = S_e / sqrt(32) / n at every position - counts every covered position exactly once.  Tolerances as in B; for a
    power-of-two n the single rounding is that of S_e * fl32(1/sqrt(32)) (the division by n is exact), so it is bit-exact."""
    g = torch.Generator().manual_seed(4000 + seed)
    v, S, meta = _counting_v(B, heads, n, cap)
    k = torch.zeros(B, heads, DH, n)
    q, _ = _one_hot_q(B, heads, n, g)
    exact = n & (n - 1) == 0
    if exact:
        want = (S.float() * torch.tensor(SCALE32, dtype=torch.float32) / n)[..., None].expand(-1, -1, -1, n)
    else:
        want = (S / math.sqrt(DH) / n)[..., None].expand(-1, -1, -1, n)
    return Case(_pack(q, k, v), _nchw(want), exact, heads, meta)


# ---------------------------------------------------------------------------------------------- Gaussian data, existing spikes
def gaussian_full(B, heads, n, seed=8):
    """The data of test_full_attention_core at any shape: N(0, 1.5^2) and one query row x 6 (online-softmax rescale)."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, 3 * heads * DH, n, generator=g) * 1.5
    qkv[B - 1, :DH, n // 2] *= 6.0
    return qkv.reshape(B, 3 * heads * DH, *hw_of(n))


def gaussian_linear(B, heads, n, seed=7):
    """The data of test_linear_attention_core at any shape: N(0, 2^2) and one k spike of 9.0 (cross-chunk max merge)."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, 3 * heads * DH, n, generator=g) * 2
    qkv[0, heads * DH + 5, (3 * n) // 4] = 9.0
    return qkv.reshape(B, 3 * heads * DH, *hw_of(n))


# ---------------------------------------------------------------------------------------------- the assertion both files use
def assert_matches(case, got, bf16):
    """`got`: the kernel's output as fp32 NCHW on the CPU.  Returns the max abs error (0.0 for the exact cases)."""
    assert got.shape == case.want.shape, (got.shape, case.want.shape)
    if case.exact:
        want = bf16_round(case.want) if bf16 else case.want
        if not torch.equal(got, want):
            bad = (got != want) | torch.isnan(got)
            first = [int(i) for i in bad.nonzero()[0]]
            raise AssertionError("%d of %d elements differ from the exact value; first at %s: got %r, want %r" % (
                int(bad.sum()), bad.numel(), first, float(got[tuple(first)]), float(want[tuple(first)])))
        return 0.0
    rel = REL_BF16 if bf16 else REL_FP32
    err = (got.double() - case.want).abs()
    ok = err <= rel * case.want.abs()                                      # NaN compares false
    if not bool(ok.all()):
        first = [int(i) for i in (~ok).nonzero()[0]]
        raise AssertionError("%d of %d elements off by more than %.3g relative; first at %s: got %r, want %r" % (
            int((~ok).sum()), ok.numel(), rel, first, float(got[tuple(first)]), float(case.want[tuple(first)])))
    return float(err.max())


# ---------------------------------------------------------------------------------------------- deliberately defective references
def _split(qkv, heads, dtype):
    b = qkv.shape[0]
    return [z.reshape(b, heads, DH, -1) for z in qkv.to(dtype).chunk(3, dim=1)]


def full_attention_slots(qkv, heads, key_idx, val_idx=None, dtype=torch.float64):
    """Softmax attention whose key slot s holds K row key_idx[s] and V row val_idx[s] (default: the same).  The identity
    list is the oracle; a shortened, lengthened or permuted one is an attention that drops, repeats or mis-pairs keys.
    dtype = float32 reproduces the single fp32 rounding that the bit-exact expectations contain."""
    val_idx = key_idx if val_idx is None else val_idx
    q, k, v = _split(qkv, heads, dtype)
    sim = torch.matmul(q.transpose(2, 3), k[..., key_idx]) * DH ** -0.5
    out = torch.matmul(sim.softmax(-1), v[..., val_idx].transpose(2, 3))   # [b, h, n, e]
    return out.transpose(2, 3).reshape(qkv.shape[0], heads * DH, *qkv.shape[2:])


def linear_attention_slots(qkv, heads, key_idx, val_idx=None, dtype=torch.float64):
    """The same for linear attention: the context sums over position slots (k from key_idx, v from val_idx); q is untouched."""
    val_idx = key_idx if val_idx is None else val_idx
    q, k, v = _split(qkv, heads, dtype)
    ctx = torch.matmul(k[..., key_idx].softmax(3), v[..., val_idx].transpose(2, 3))
    out = torch.matmul(ctx.transpose(2, 3), q.softmax(2) * DH ** -0.5)
    return out.reshape(qkv.shape[0], heads * DH, *qkv.shape[2:])


def defect_slots(n, defect, j, j2=None):
    """(key_idx, val_idx) of an attention with one defect at key / position j: "drop" loses it, "dup" counts it twice,
    "swap" pairs keys j and j2 with each other's V rows."""
    ident = list(range(n))
    if defect == "drop":
        idx = ident[:j] + ident[j + 1:]
        return idx, idx
    if defect == "dup":
        idx = ident[:j + 1] + ident[j:]
        return idx, idx
    assert defect == "swap" and j2 is not None and j2 != j
    val = list(ident)
    val[j], val[j2] = val[j2], val[j]
    return ident, val


# ---------------------------------------------------------------------------------------------- shapes: one row per dispatch branch
# (group, element type, B, heads, n).  group = the kernel that full_attention() / linear_attention() choose for that shape:
#   scalar  n % 32 != 0: full_attn_kernel (64-key LDS tiles, blocks of 16, ragged tail; n = 1000 is a 4-block grid with an
#           inactive tail, tc = 1, 17, 35, 36, 40 at the last tile)
#   mfma    n % 32 == 0: full_attn_mfma_kernel (bf16 only above the LDS kernel's limit)
#   lds     bf16, n % 256 == 0, n <= 1024: full_attn_bf16_kernel
#   linear  la_partial / la_combine / la_apply; chunk length 512 up to n = 16384, 1024 above (16448 leaves a ragged 1024-chunk)
FULL_SHAPES = (
    [("scalar", t, *s) for t in ("fp32", "bf16") for s in [(1, 4, 1), (3, 1, 17), (2, 8, 99), (2, 4, 100), (1, 4, 1000)]]
    + [("mfma", "fp32", *s) for s in [(3, 8, 32), (1, 1, 96), (2, 4, 1024), (1, 4, 4096)]]
    + [("mfma", "bf16", *s) for s in [(3, 8, 1280), (1, 1, 4096)]]
    + [("lds", "bf16", *s) for s in [(3, 4, 256), (1, 8, 512), (2, 1, 768), (2, 4, 1024)]]
)
LINEAR_SHAPES = [("linear", t, *s) for t in ("fp32", "bf16")
                 for s in [(3, 4, 4), (2, 1, 100), (1, 4, 512), (2, 4, 516), (3, 8, 1023), (1, 4, 16384), (2, 4, 16448), (1, 4, 65536)]]


def shape_id(s):
    return "%s-%s-B%d-h%d-N%d" % s


def cap_of(elem):
    return CAP_BF16 if elem == "bf16" else CAP_FP32
