"""Closed-form and float64 cases for the fused bf16 LinearAttention block (linattn_fused.hip, linattn_fused256.hip:
la1 -> la_combine -> la2).  Pure torch on the CPU; tests/test_linattn_block_cases_cpu.py proves the cases, and
tests/test_linattn_block_exact_gpu.py feeds them to the kernels.

Every input goes through the block's real interface (x, to_qkv, norm.g, to_out weight / bias, to_out.1.g) and is exact in bf16.
The gains are chosen so that the host-side fold W * (g * sqrt(C)) is a bf16 value again: g = 2^j / 16 at C = 256 and
g = fp32(2^j / sqrt(128)) at C = 128, so the reference and the kernel consume the same weights.

The expected y is oracle.srgd_oracle.linear_attention in float64 plus x (`expected`); the expected normalised context and row norms
come from `reference`, the same arithmetic written out (the CPU test holds the two together).

Families (`make_case(family, C, N)`):
  count     W_k = W_q = 0: both softmaxes are uniform, every context row is scale * mean_n v[e, n], the attention output is the same
            for every pixel.  x carries a tile code and a strip code (one channel each, +4), so each (tile, e) pair has its own
            weight in the mean; the to_out bias is of the order of the attention output, so a uniform scale error survives the
            second RMSNorm.
  select    k is one-hot over positions per column (level channels 0..31 for d, 32..35 for the head, both read with weight 1024: the
            runner-up is > 150 below in the log2 domain, its exponential is 0 in fp32), q is one-hot over d (level channels 36..67).
            The selected positions lie in the first tile, in the last 64 positions and in between, and differ per head and per d.
            The context is one v row, the output pairs them through q.  Every fourth pixel has a runner-up 1/16 below its level
            and the odd tiles have twice the norm: there q' is a two-way mix whose weights depend on the pixel's own 1 / ||x||.
  lazy      per-tile column maxima follow a script in the log2 domain.  Row d of a scripted tile carries the peak of column d of
            head 0 (level channel d) and of head 1 (level channel 32 + d); all other rows sit at k = 0.  Head 0, by column class
            d % 4: a rise of 7.6 (the reference point must not move, p reaches 2^7.6), of 8.4, of 44, and a fall of 35 - at the
            second tile of every strip, at the last tile of a ragged last strip, and (odd strips) at the first tile of the strip,
            which is the combine path.  Head 1: all 32 columns jump by 8.25 + 0.12 d in the second tile of every strip (and by
            8.25 + 0.12 (31 - d) in the last tile of a ragged strip): one rescale applies 32 different factors.  The peak rows of
            those tiles have v = 0 in head 1, so the rescaled old context is the whole of the new one.  Heads 2 and 3 hold still.
  gaussian  the data of the older parity test (x ~ 1.5 N(0, 1), weights ~ N(0, 1 / fan_in), all rounded to bf16) plus one level
            spike (x = 64 in channel 0 of a position in the last tile of a strip, read by k column 3 of head 0 with weight 16).  The accuracy yardstick.

`emulate` is a CPU emulation of the block: float64 arithmetic, values rounded to bf16 where the kernels make them bf16 -
  1. the folded weights Wq', Wkv' (fp32 product W * (g * sqrt(C)), then bf16) and Wout           (linattn_fused*_pack)
  2. p = exp2(k - m) and v / ||x|| when they become the operands of the context product           (la1: pack8 of k0/k1, v0/v1);
     the column sums l add the unrounded p
  3. the normalised context and the normalised q' when they become the operands of att            (la2: cx[], pack8 of q0/q1)
  4. the attention tile in LDS                                                                     (la2: pack4 / (bf16)a0[..] -> sT)
  5. C = 128 only: RMSNorm(o) * g2 staged in LDS before the residual is added                      (la2: pack4 -> sT)
  6. y                                                                                             (la2: (bf16)(.. + x))
and with the kernels' own schedule: 64-pixel tiles at C = 128, 32-pixel tiles at C = 256, strips of `design_strip(N)` pixels, the
lazy reference point (moved only by a tile maximum more than 8 above it), one partial per strip, merged as la_combine does.
Everything the kernels keep in fp32 stays float64 here.  `emulate(case, mutant)` also builds the thirteen wrong variants (MUTANTS).

Gates.  Per family, per C and per checked tensor the gate of an element is  a * 2^-9 * |want| + b.  (a, b) are fitted to the
emulation's error against the float64 reference over SHAPES_CPU (`fit_gate`): a = twice the worst error / (2^-9 |want|) over the
elements with |want| >= max|want| / 2, b = twice what that leaves uncovered on the smaller elements; then the floors below.  The
kernel's output is never used.  Floors, from the number formats:
  y      a >= 4: 4 * 2^-9 |want| = 2^-7 |want| >= one bf16 ulp of the output
  ctxn   a >= 2^-8 (fp32 arithmetic on ~100-term sums), b >= 2^-20 max|want| (fp32 cancellation in v and in the merged strips)
  rinv   a >= (C + 8) * 2^-24 / 2^-9: C fp32 additions of positive squares, a square root and a division; b = 0
Measured on the CPU (emulation error in units of the final gate, i.e. <= 0.5 where the fit and not a floor decides; GATES holds
the fitted values rounded up to two digits):
  count     C = 128  y     fitted a = 4         b = 0.001048   -> gate a = 4        b = 0.0011
  count     C = 128  ctxn  fitted a = 0.5816    b = 4.796e-05  -> gate a = 0.59     b = 4.8e-05
  count     C = 128  rinv  fitted a = 0.00415   b = 0          -> gate a = 0.0042   b = 0
  select    C = 128  y     fitted a = 4         b = 0.00338    -> gate a = 4        b = 0.0034
  select    C = 128  ctxn  fitted a = 3.977     b = 2.761e-07  -> gate a = 4        b = 2.8e-07
  select    C = 128  rinv  fitted a = 0.00415   b = 0          -> gate a = 0.0042   b = 0
  lazy      C = 128  y     fitted a = 4         b = 0.003986   -> gate a = 4        b = 0.004
  lazy      C = 128  ctxn  fitted a = 4.78      b = 4.833e-07  -> gate a = 4.8      b = 4.9e-07
  lazy      C = 128  rinv  fitted a = 0.00415   b = 0          -> gate a = 0.0042   b = 0
  gaussian  C = 128  y     fitted a = 4         b = 0.003786   -> gate a = 4        b = 0.0038
  gaussian  C = 128  ctxn  fitted a = 3.113     b = 4.392e-05  -> gate a = 3.2      b = 4.4e-05
  gaussian  C = 128  rinv  fitted a = 0.00415   b = 0          -> gate a = 0.0042   b = 0
  count     C = 256  y     fitted a = 4         b = 0.0009314  -> gate a = 4        b = 0.00094
  count     C = 256  ctxn  fitted a = 0.5083    b = 5.172e-05  -> gate a = 0.51     b = 5.2e-05
  count     C = 256  rinv  fitted a = 0.008057  b = 0          -> gate a = 0.0081   b = 0
  select    C = 256  y     fitted a = 4         b = 0.002623   -> gate a = 4        b = 0.0027
  select    C = 256  ctxn  fitted a = 3.715     b = 6.033e-05  -> gate a = 3.8      b = 6.1e-05
  select    C = 256  rinv  fitted a = 0.008057  b = 0          -> gate a = 0.0081   b = 0
  lazy      C = 256  y     fitted a = 4         b = 0.00154    -> gate a = 4        b = 0.0016
  lazy      C = 256  ctxn  fitted a = 5.469     b = 6.619e-07  -> gate a = 5.5      b = 6.7e-07
  lazy      C = 256  rinv  fitted a = 0.008057  b = 0          -> gate a = 0.0081   b = 0
  gaussian  C = 256  y     fitted a = 4         b = 2.416e-05  -> gate a = 4        b = 2.5e-05
  gaussian  C = 256  ctxn  fitted a = 3.422     b = 2.424e-05  -> gate a = 3.5      b = 2.5e-05
  gaussian  C = 256  rinv  fitted a = 0.008057  b = 0          -> gate a = 0.0081   b = 0
"""
import math

import torch

LOG2E = 1.4426950408889634
SCALE = 32 ** -0.5
FAMILIES = ("count", "select", "lazy", "gaussian")
TENSORS = ("y", "ctxn", "rinv")
SHAPES_CPU = (64, 128, 192, 256, 320, 576, 1088, 2112, 16576, 65600)        # every N of the GPU test
MUTANTS = ("drop_position", "tile_twice", "skip_last_ragged_tile", "rescale_wrong_row", "move_without_rescaling_l",
           "strip_wrong_max", "swap_v_rows", "swap_head_contexts", "rinv_from_next_tile", "q_softmax_31", "no_bias",
           "residual_from_next_tile", "rms2_missing_block")
F64 = torch.float64


def bf(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def tile_px(C):
    return 64 if C == 128 else 32


def design_strip(N):
    """The la1 strip length the cases are designed for; the GPU test checks it against what the launcher reports."""
    return 2048 if N >= 65536 else 1024 if N >= 16384 else 512 if N >= 2048 else 256


def gain_unit(C, j):
    """g (fp32) with g * sqrt(C) = 2^j up to fp32 rounding: W * (g * sqrt(C)) is W * 2^j again once it is rounded to bf16."""
    j = torch.as_tensor(j, dtype=F64)
    return (2.0 ** j / 16.0).float() if C == 256 else (2.0 ** j / math.sqrt(128.0)).float()


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _params(C, g, jq=None):
    """Generic bf16-exact weights; the families overwrite what they script."""
    P = {"C": C}
    P["wqkv"] = _ints(g, (384, C), -8, 8) / 8.0
    P["g1"] = gain_unit(C, torch.zeros(C) if jq is None else jq)
    P["wout"] = _ints(g, (C, 128), -16, 16) / 16.0
    P["bout"] = torch.zeros(C, dtype=F64)
    P["g2"] = gain_unit(C, _ints(g, (C,), 0, 1))
    return P


def _set_bias(P, x, g):
    """to_out bias of the order of the attention output (so that a uniform scale error survives RMSNorm2), exact in bf16."""
    r = reference(x, P)
    s = float(r["o_nobias"].abs().mean())
    P["bout"] = bf(torch.randn(P["C"], generator=g).to(F64) * s)


def folded(P):
    """The host's fold, as linattn_fused*_pack does it: fp32 product, then bf16."""
    C = P["C"]
    gs = P["g1"].float() * torch.tensor(float(C)).sqrt()
    return (P["wqkv"].float() * gs[None, :]).to(torch.bfloat16).to(F64)


# ----------------------------------------------------------------------------------------------------------- reference
def reference(x, P, dtype=F64):
    """The block in `dtype`, written out: y, ctxn (normalised context * dim_head^-0.5, [4][32 d][32 e]) and rinv."""
    C = P["C"]
    x = x.to(dtype)
    N = x.shape[0]
    nrm = x.pow(2).sum(1).sqrt().clamp_min(1e-12)
    xn = x / nrm[:, None] * P["g1"].to(dtype) * (C ** 0.5)
    qkv = xn @ P["wqkv"].to(dtype).T
    q, k, v = [z.reshape(N, 4, 32) for z in qkv.split(128, dim=1)]
    qs = q.softmax(dim=2)
    ks = k.softmax(dim=0)
    ctx = torch.einsum("nhd,nhe->hde", ks, v)
    att = torch.einsum("hde,nhd->nhe", ctx, qs * SCALE).reshape(N, 128)
    o_nb = att @ P["wout"].to(dtype).T
    o = o_nb + P["bout"].to(dtype)
    y = o / o.pow(2).sum(1).sqrt().clamp_min(1e-12)[:, None] * P["g2"].to(dtype) * (C ** 0.5) + x
    return {"y": y, "ctxn": ctx * SCALE, "rinv": 1.0 / nrm, "o_nobias": o_nb, "k_log2": k * LOG2E, "v": v}


def state_dict(P, dtype=F64):
    C = P["C"]
    return {"a.norm.g": P["g1"].to(dtype).reshape(1, C, 1, 1), "a.to_qkv.weight": P["wqkv"].to(dtype).reshape(384, C, 1, 1),
            "a.to_out.0.weight": P["wout"].to(dtype).reshape(C, 128, 1, 1), "a.to_out.0.bias": P["bout"].to(dtype),
            "a.to_out.1.g": P["g2"].to(dtype).reshape(1, C, 1, 1)}


def oracle_y(x, P, dtype=F64):
    """oracle.srgd_oracle.linear_attention (+ x) on the same tensors: x [N, C] -> y [N, C]."""
    from oracle import srgd_oracle as O
    xi = x.to(dtype).T.reshape(1, P["C"], x.shape[0], 1)
    y = O.linear_attention(state_dict(P, dtype), "a", xi, 4, 32) + xi
    return y.reshape(P["C"], x.shape[0]).T.contiguous()


def expected(case):
    """float64 expectations of a case: y from the oracle, ctxn and rinv from `reference`."""
    r = reference(case["x"], case["P"])
    return {"y": oracle_y(case["x"], case["P"]), "ctxn": r["ctxn"], "rinv": r["rinv"]}


# ----------------------------------------------------------------------------------------------------------- emulation
def emulate(case, mutant=None):
    """The kernels' arithmetic and schedule on the CPU (module docstring); `mutant` in MUTANTS builds a wrong variant."""
    assert mutant is None or mutant in MUTANTS
    x, P, H = case["x"], case["P"], case["hints"]
    C, N = P["C"], x.shape[0]
    TM, strip = tile_px(C), design_strip(N)
    Wf = folded(P)
    rinv = 1.0 / x.pow(2).sum(1).sqrt().clamp_min(1e-12)
    kv = x @ Wf[128:].T
    k = (kv[:, :128] * (rinv * LOG2E)[:, None]).reshape(N, 4, 32)
    v = (kv[:, 128:] * rinv[:, None]).reshape(N, 4, 32)
    if mutant == "swap_v_rows":
        n1, n2 = H["v_rows"]
        v = v.clone()
        v[[n1, n2]] = v[[n2, n1]]
    ntiles = N // TM
    last_ragged = ntiles - 1 if N % strip else -1
    swap4 = torch.arange(32) ^ 4
    pm, pl, pc, trace = [], [], [], []
    for s0 in range(0, N, strip):
        m = torch.full((4, 32), -math.inf, dtype=F64)
        l = torch.zeros(4, 32, dtype=F64)
        ctx = torch.zeros(4, 32, 32, dtype=F64)
        for p0 in range(s0, min(s0 + strip, N), TM):
            t = p0 // TM
            if mutant == "skip_last_ragged_tile" and t == last_ragged:
                continue
            kt, vt = k[p0:p0 + TM], v[p0:p0 + TM]
            bm = kt.max(0).values
            mn = torch.where(bm > m + 8.0, bm, m)
            f = torch.exp2(m - mn)
            trace.append({"tile": t, "first": p0 == s0, "rise": bm - m, "f": f})
            m = mn
            p = torch.exp2(kt - mn)
            if mutant == "drop_position" and p0 <= H["position"] < p0 + TM:
                p = p.clone()
                p[H["position"] - p0] = 0
            reps = 2 if (mutant == "tile_twice" and t == H["tile"]) else 1
            for rep in range(reps):
                fr = f if rep == 0 else torch.ones_like(f)
                if mutant != "move_without_rescaling_l":
                    l = l * fr
                l = l + p.sum(0)
                ctx = ctx * (fr[:, swap4] if mutant == "rescale_wrong_row" else fr)[:, :, None]
                ctx = ctx + torch.einsum("nhd,nhe->hde", bf(p), bf(vt))
        pm.append(m)
        pl.append(l)
        pc.append(ctx)
    pm, pl, pc = torch.stack(pm), torch.stack(pl), torch.stack(pc)           # [strips][4][32](...)
    M = pm.max(0).values
    w = torch.exp2(pm - M)                                                    # (la_combine: exp(m ln2 - M ln2))
    if mutant == "strip_wrong_max" and pm.shape[0] > 1:
        w = torch.exp2(torch.roll(pm, 1, 0) - M)
    ctxn = (pc * w[..., None]).sum(0) * (SCALE / (pl * w).sum(0))[..., None]
    if mutant == "swap_head_contexts":
        ctxn = ctxn[[0, 2, 1, 3]]
    # ---- la2
    nxt = (torch.arange(N) + TM) % N
    q = (x @ Wf[:128].T).reshape(N, 4, 32)
    ri = (rinv[nxt] if mutant == "rinv_from_next_tile" else rinv) * LOG2E
    e = torch.exp2((q - q.max(2, keepdim=True).values) * ri[:, None, None])
    ssum = e[:, :, :31].sum(2) if mutant == "q_softmax_31" else e.sum(2)
    qn = e / ssum[:, :, None]
    att = bf(torch.einsum("hde,nhd->nhe", bf(ctxn), bf(qn))).reshape(N, 128)
    o = att @ bf(P["wout"]).T
    if mutant != "no_bias":
        o = o + P["bout"]
    sq = o.pow(2)
    if mutant == "rms2_missing_block":
        sq = sq[:, C // 4:]
    rn = 1.0 / sq.sum(1).sqrt().clamp_min(1e-12)
    g2s = (P["g2"].float() * torch.tensor(float(C)).sqrt()).to(F64)
    xr = x[nxt] if mutant == "residual_from_next_tile" else x
    on = o * rn[:, None] * g2s
    y = bf(bf(on) + xr) if C == 128 else bf(on + xr)
    return {"y": y, "ctxn": ctxn, "rinv": rinv, "trace": trace}


# ----------------------------------------------------------------------------------------------------------- families
def _hints(N, C, position=None):
    TM = tile_px(C)
    position = N - 5 if position is None else position
    return {"position": position, "v_rows": (position, position ^ 1), "tile": 1 if N // TM > 1 else 0}


def _count(C, N, g):
    TM, strip = tile_px(C), design_strip(N)
    P = _params(C, g)
    P["wqkv"][:256] = 0
    x = _ints(g, (N, C), 0, 3)
    n = torch.arange(N)
    x[n, (n // TM) % 64] += 4
    x[n, 64 + (n // strip) % 32] += 4
    _set_bias(P, x, g)
    return x, P, _hints(N, C)


def select_position(N, h, d):
    """The position column d of head h selects."""
    idx = h * 32 + d
    if N < 192:
        return idx % N
    if idx < 32:
        return 2 * idx + 1
    if idx < 64:
        return N - 1 - 2 * (idx - 32)
    return 64 + ((idx - 64) * 61) % (N - 128)


def select_q(n, h):
    """The column d pixel n selects in head h."""
    return ((5 * n + 1) % 32 - 8 * h) % 32


def _select(C, N, g):
    P = _params(C, g)
    P["wqkv"][:256] = 0
    P["wqkv"][256:, :68] = 0
    x = torch.zeros(N, C, dtype=F64)
    n = torch.arange(N)
    x[:, 68:] = _ints(g, (N, C - 68), -2, 2) * (1 + (n // tile_px(C)) % 2)[:, None]      # odd tiles: twice the norm
    x[n, 36 + (5 * n + 1) % 32] = 8
    soft = n[n % 4 == 2]                                  # every fourth pixel: a runner-up 1/16 below, so q' is a two-way mix
    x[soft, 36 + (5 * soft + 2) % 32] = 7.9375            # whose weights depend on the pixel's own 1 / ||x||
    for h in range(4):
        for d in range(32):
            ns = select_position(N, h, d)
            x[ns, d] = 16
            x[ns, 32 + h] = 16
            P["wqkv"][128 + h * 32 + d, d] = 1024
            P["wqkv"][128 + h * 32 + d, 32 + h] = 1024
            P["wqkv"][h * 32 + d, 36 + (d + 8 * h) % 32] = 1024
    _set_bias(P, x, g)
    return x, P, _hints(N, C, select_position(N, 1, 5))


LAZY_W = 128.0                                           # folded weight of a level channel
LAZY_BASE, LAZY_DELTA = (2.0, 2.0, 2.0, 46.0), (7.6, 8.4, 44.0, -35.0)


def lazy_jump(d):
    return 8.25 + 0.12 * d


def lazy_script(C, N):
    """Target tile maxima (log2 domain) K[tile][head 0 / 1][d]; 0 = no peak (the tile's rows all sit at k = 0)."""
    TM, strip = tile_px(C), design_strip(N)
    ntiles, tps = N // TM, strip // TM
    d = torch.arange(32)
    B = torch.tensor([LAZY_BASE[i % 4] for i in range(32)], dtype=F64)
    D = torch.tensor([LAZY_DELTA[i % 4] for i in range(32)], dtype=F64)
    J = lazy_jump(d.to(F64))
    K = torch.zeros(ntiles, 2, 32, dtype=F64)
    for t in range(ntiles):
        s, ti = t // tps, t % tps
        T = min(tps, ntiles - s * tps)
        b0 = B + D * (s % 2)
        b1 = 1.0 + 0.05 * d + 3.0 * (s % 2)
        m0 = torch.where((D > 8) & (T > 1), b0 + D, b0)                 # the reference points after the second tile
        m1 = b1 + J if T > 1 else b1
        if ti == 0:
            K[t, 0], K[t, 1] = b0, b1
        elif ti == 1:
            K[t, 0], K[t, 1] = (b0 + D).clamp_min(0), b1 + J
        elif t == ntiles - 1 and T < tps:
            K[t, 0], K[t, 1] = (m0 + D).clamp_min(0), m1 + J.flip(0)
    return K


def _lazy(C, N, g):
    TM, strip = tile_px(C), design_strip(N)
    tps = strip // TM
    bal, va, vb = (64, 80, 104) if C == 128 else (64, 128, 192)
    P = _params(C, g)
    P["wqkv"][:, :va] = 0                                 # q, k, v read the value channels only ...
    P["wqkv"][128:256] = 0                                # ... k reads nothing but its level channel (heads 2, 3: nothing)
    for h in range(4):                                    # heads 0, 2 take v from value set B, heads 1, 3 from value set A
        rows = slice(256 + h * 32, 256 + h * 32 + 32)
        if h % 2 == 0:
            P["wqkv"][rows, va:vb] = 0
        else:
            P["wqkv"][rows, vb:] = 0
    for d in range(32):
        P["wqkv"][128 + d, d] = LAZY_W
        P["wqkv"][128 + 32 + d, 32 + d] = LAZY_W
    x = torch.zeros(N, C, dtype=F64)
    x[:, bal:va] = _ints(g, (N, va - bal), 0, 1) * 2 - 1
    x[:, va:] = _ints(g, (N, C - va), 0, 3)               # v >= 0 throughout: no cancellation in the context sums, so the
    P["wqkv"][256:, va:] = P["wqkv"][256:, va:].abs()     # rescaled rows of head 1 stay far above the rounding noise of the rest
    K = lazy_script(C, N)
    W = LAZY_W * LOG2E
    for t in range(K.shape[0]):
        if not bool((K[t] != 0).any()):
            continue
        rows = torch.arange(t * TM, t * TM + 32)
        ti = t % tps
        if ti >= 1:                                       # head 1's rescale tiles: its v is 0 on the peak rows
            x[rows, va:vb] = 0
        F = x[rows].pow(2).sum(1)
        R = (F / (1.0 - (K[t, 0] ** 2 + K[t, 1] ** 2) / W ** 2)).sqrt()
        x[rows, torch.arange(32)] = bf(K[t, 0] * R / W)
        x[rows, 32 + torch.arange(32)] = bf(K[t, 1] * R / W)
    _set_bias(P, x, g)
    return x, P, _hints(N, C, (TM + 1) if N > TM else 1)


def _gaussian(C, N, g):
    P = {"C": C}
    jq = _ints(g, (C,), -1, 1)
    P["wqkv"] = bf(torch.randn(384, C, generator=g).to(F64) / C ** 0.5)
    P["g1"] = gain_unit(C, jq)
    P["wout"] = bf(torch.randn(C, 128, generator=g).to(F64) / 128 ** 0.5)
    P["bout"] = bf(0.1 * torch.randn(C, generator=g).to(F64))
    P["g2"] = gain_unit(C, _ints(g, (C,), 0, 1))
    x = bf(torch.randn(N, C, generator=g).to(F64) * 1.5)
    rag = N % design_strip(N)
    spike = N - 5 if rag == 0 or rag > tile_px(C) else N - rag - 5     # never in the first tile of a strip (where N allows)
    x[spike, 0] = 64
    P["wqkv"][128 + 3, 0] = bf(16.0 / 2.0 ** jq[0])
    return x, P, _hints(N, C, spike)


_BUILD = {"count": _count, "select": _select, "lazy": _lazy, "gaussian": _gaussian}
_CACHE = {}


def make_case(family, C, N):
    """One case: x [N, C] float64 (bf16-exact), P (the block's weights, bf16-exact, gains fp32) and the mutants' hints."""
    key = (family, C, N)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * FAMILIES.index(family) + C + N)
        x, P, H = _BUILD[family](C, N, g)
        _CACHE[key] = {"family": family, "C": C, "N": N, "x": x, "P": P, "hints": H}
    return _CACHE[key]


# ----------------------------------------------------------------------------------------------------------- gates
def gate_floor(tensor, C):
    """(a_min, b_min as a fraction of max|want|): module docstring."""
    if tensor == "y":
        return 4.0, 0.0
    if tensor == "ctxn":
        return 2.0 ** -8, 2.0 ** -20
    return (C + 8) * 2.0 ** -24 / 2.0 ** -9, 0.0


def fit_gate(errs_wants, tensor, C):
    """(a, b, b / max|want|) from the emulation's errors over a family's cases: twice the worst error, then the floors."""
    a = b = 0.0
    wmax = max(float(w.abs().max()) for _, w in errs_wants)
    for err, want in errs_wants:
        u = 2.0 ** -9 * want.abs()
        big = want.abs() >= 0.5 * wmax
        if bool(big.any()):
            a = max(a, 2.0 * float((err[big] / u[big]).max()))
    a_min, b_min = gate_floor(tensor, C)
    a = max(a, a_min)
    for err, want in errs_wants:
        b = max(b, 2.0 * float((err - 0.5 * a * 2.0 ** -9 * want.abs()).clamp_min(0).max()))
    return a, max(b, b_min * wmax)


def gate(family, C, tensor, want):
    a, b = GATES[(family, C, tensor)]
    return a * 2.0 ** -9 * want.abs() + b


def excess(got, want, family, C, tensor):
    """Worst element of |got - want| in units of its gate (<= 1 passes), and the worst absolute error."""
    err = (got.to(F64) - want).abs()
    ratio = torch.nan_to_num(err / gate(family, C, tensor, want), nan=math.inf)          # a NaN never passes
    return float(ratio.max()), float(torch.nan_to_num(err, nan=math.inf).max())


# (family, C, tensor) -> (a, b): fitted by tools in this module (fit_gate over SHAPES_CPU), rounded up to two digits
GATES = {
    ("count", 128, "y"): (4.0, 0.0011),
    ("count", 128, "ctxn"): (0.59, 4.8e-05),
    ("count", 128, "rinv"): (0.0042, 0.0),
    ("select", 128, "y"): (4.0, 0.0034),
    ("select", 128, "ctxn"): (4.0, 2.8e-07),
    ("select", 128, "rinv"): (0.0042, 0.0),
    ("lazy", 128, "y"): (4.0, 0.004),
    ("lazy", 128, "ctxn"): (4.8, 4.9e-07),
    ("lazy", 128, "rinv"): (0.0042, 0.0),
    ("gaussian", 128, "y"): (4.0, 0.0038),
    ("gaussian", 128, "ctxn"): (3.2, 4.4e-05),
    ("gaussian", 128, "rinv"): (0.0042, 0.0),
    ("count", 256, "y"): (4.0, 0.00094),
    ("count", 256, "ctxn"): (0.51, 5.2e-05),
    ("count", 256, "rinv"): (0.0081, 0.0),
    ("select", 256, "y"): (4.0, 0.0027),
    ("select", 256, "ctxn"): (3.8, 6.1e-05),
    ("select", 256, "rinv"): (0.0081, 0.0),
    ("lazy", 256, "y"): (4.0, 0.0016),
    ("lazy", 256, "ctxn"): (5.5, 6.7e-07),
    ("lazy", 256, "rinv"): (0.0081, 0.0),
    ("gaussian", 256, "y"): (4.0, 2.5e-05),
    ("gaussian", 256, "ctxn"): (3.5, 2.5e-05),
    ("gaussian", 256, "rinv"): (0.0081, 0.0),
}
