"""Closed-form cases for the conditioning path: srgd_amd/csrc/cond.hip (``time_features``, ``linear_rows``), ``compute_conditioning``
in engine.hip, and the row addressing of ``gn_finalize`` (norm_act.hip).  CPU only: constructions, float64 references, tolerances
derived from the oracle alone, and mutants.  tests/test_cond_cases_cpu.py proves the constructions and shows that every assertion
rejects every mutant; tests/test_cond_exact_gpu.py feeds the cases to the kernels through the read-only probes of
include/srgd_hip_kernels.h (srgd_k_time_features, srgd_k_linear_rows, srgd_k_conditioning_table / _layout, srgd_k_gn_coefficients).

Two exactness devices (fp32, asserted on the CPU):
  * SiLU is the identity or zero: t >= 32 -> t (1 + exp(-t) == 1), t <= -96 -> -0 (exp(-t) = inf), silu(0) = 0.
  * erf-GELU is the identity or zero: gelu(s) = s for s >= 16, -0 for s <= -16, gelu(0) = 0, because erff(|s| / sqrt 2) == 1.
With small-integer weights and inputs that keep every pre-SiLU value in {0} u [32, inf) u (-inf, -96] and every pre-GELU value a
multiple of 16, every result is an integer below 2^24: the same in any summation order, with or without FMA contraction, and
compared BIT FOR BIT (-0 == +0).  ``designed_state_dict`` builds such a network; ``designed_trace`` asserts the sets.

The designed table.  time_mlp.0.weights = 0, so the features of log-SNR x are [x, 0 x 16, 1 x 16].  Hidden units of the time MLP:
h1 = [16 x, 16 (a cos feature), 32 (a sin feature, 0, plus bias 32), gelu(-16 x) = -0, 0 ...]; t = [32 + 16 x, 32, -96, 0, 0, ...];
the class embedding of label l adds 32 (l + 1) to unit 4.  After SiLU: s = [32 + 16 x, 32, 0, 0, 32 (l + 1) | 0 (null row), ...].
Column g (counted over blocks in state-dict order, scale half before shift half, channel by channel) of the table is
    g + 524288 (g % 7) + 16384 (2 + x) + 131072 (l + 1 | 0):  bias g, weights 16384 (g % 7) on unit 1, 1024 on unit 0, 4096 on unit 4
(and 7 on unit 2, 5 on unit 3, which contribute 0) - four fields that do not overlap, so every entry names its log-SNR value, its
label or the null row, its block, half and channel, and no two entries of a table are equal.

How much the existing end-to-end gate would miss (tests/test_cond_cases_cpu.py -s; oracle in fp32, dim 16, sample 0 of the ``dim16_128``
fixture's inputs cropped to 64 x 64, max |eps - eps'| of ONE forward pass at three steps of the 50-step DDPM run; the gate of
test_unet_forward_matches_reference is 1e-4 * scale = 1.4e-4 here):
    step (log-SNR)    neighbouring step's row   label <-> null row   scale <-> shift
     1 (-9.604)       0.291 = 1950 x gate       0.263 = 1760 x       0.358 = 2400 x
    25 (-2.414)       0.127 =  925 x            0.217 = 1580 x       0.207 = 1500 x
    48 (+4.121)       0.229 = 1640 x            0.244 = 1740 x       0.206 = 1470 x
On the random weights a wholly wrong row is visible to that gate by three orders of magnitude; it decides nothing here.  What the gate
cannot do is name the wrong term, and it never runs K > 1, step values above the fixtures' few, or a stride that differs from the
row width.
"""
import functools
import json
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import srgd_oracle as O
from srgd_amd.synth import synth_state_dict

G = os.path.join(os.path.dirname(__file__), "golden")
MARGIN = 8
FLOOR_ULPS = 4
MUTANT_FACTOR = 100
HALF = 16                        # learned_sinusoidal_dim / 2
GUARD = 32
PI32 = float(np.float32(math.pi))


def ulp32(v: float) -> float:
    return 2.0 ** (math.floor(math.log2(v)) - 23) if v > 0 else 2.0 ** -149


def distance(a, b) -> float:
    d = (a.double() - b.double()).abs()
    return float("inf") if not bool(torch.isfinite(d).all()) else float(d.max())


def exact_factor(mutant, want) -> float:
    """An exact assertion admits no error; a mutant's factor against it is its largest error in fp32 ulps of the largest expected
    magnitude (a lower bound of the error in the element's own ulps)."""
    return distance(mutant, want) / ulp32(float(want.abs().max()))


def assert_exact(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.double() != want.double()
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %r, want %r" % (what, int(bad.sum()), bad.numel(), i, float(got[i]), float(want[i])))


def assert_devices():
    """The two exactness devices in fp32 on the CPU."""
    t = torch.tensor([32.0, 48.0, 96.0, 1e4])
    z = torch.tensor([-96.0, -100.0, -1e4])
    assert torch.equal(F.silu(t), t) and torch.equal(t / (1 + torch.exp(-t)), t)
    assert not F.silu(z).any() and not (z / (1 + torch.exp(-z))).any() and float(F.silu(torch.zeros(1))) == 0.0
    s = torch.tensor([16.0, 32.0, 48.0, 8192.0])
    assert torch.equal(F.gelu(s), s) and not F.gelu(-s).any() and float(F.gelu(torch.zeros(1))) == 0.0
    assert torch.equal(0.5 * s * (1 + torch.erf(s * 0.70710678118654752440)), s)


# ------------------------------------------------------------------------------------------------ schema
def schema(dim) -> Dict[str, tuple]:
    with open(os.path.join(G, f"schema_dim{dim}.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


def blocks(dim) -> List[tuple]:
    """(state-dict prefix without "model.", Cout) of every ResnetBlock, in state-dict order."""
    return [(k[len("model."):-len(".mlp.1.bias")], v[0] // 2) for k, v in schema(dim).items() if k.endswith(".mlp.1.bias")]


def strip(sd):
    return O.strip_model_prefix(sd)


# ------------------------------------------------------------------------------------------------ 1. the designed table
X_UNIT, COS_UNIT, SIN_UNIT, NEG_UNIT, LABEL_UNIT = 0, 1, 2, 3, 4
W_X, W_LABEL, W_COL = 1024, 4096, 16384


def designed_state_dict(dim) -> Dict[str, torch.Tensor]:
    """``synth_state_dict`` with the conditioning tensors replaced (module docstring); keys carry the "model." prefix."""
    sc = schema(dim)
    sd = synth_state_dict(sc, seed=0)
    z = lambda k: torch.zeros(sc["model." + k])
    w0 = z("time_mlp.0.weights")
    w1, b1 = z("time_mlp.1.weight"), z("time_mlp.1.bias")
    w1[X_UNIT, 0] = 16
    w1[COS_UNIT, 1 + HALF] = 16
    w1[SIN_UNIT, 1] = 16
    b1[SIN_UNIT] = 32
    w1[NEG_UNIT, 0] = -16
    w3, b3 = z("time_mlp.3.weight"), z("time_mlp.3.bias")
    w3[X_UNIT, X_UNIT] = 1
    b3[X_UNIT] = 32
    w3[COS_UNIT, COS_UNIT] = 2
    w3[SIN_UNIT, SIN_UNIT] = -3
    w3[NEG_UNIT, NEG_UNIT] = 9
    emb = z("class_mlp.0.weight")
    c1, cb1 = z("class_mlp.1.weight"), z("class_mlp.1.bias")
    c3, cb3 = z("class_mlp.3.weight"), z("class_mlp.3.bias")
    for l in range(emb.shape[0]):
        emb[l, l] = 1
        c1[l, l] = 16 * (l + 1)
        c3[LABEL_UNIT, l] = 2
    new = {"time_mlp.0.weights": w0, "time_mlp.1.weight": w1, "time_mlp.1.bias": b1, "time_mlp.3.weight": w3, "time_mlp.3.bias": b3,
           "class_mlp.0.weight": emb, "class_mlp.1.weight": c1, "class_mlp.1.bias": cb1, "class_mlp.3.weight": c3, "class_mlp.3.bias": cb3}
    g0 = 0
    for name, cout in blocks(dim):
        w, b = z(name + ".mlp.1.weight"), z(name + ".mlp.1.bias")
        g = torch.arange(g0, g0 + 2 * cout)
        b[:] = g.float()
        w[:, X_UNIT] = W_X
        w[:, COS_UNIT] = (W_COL * (g % 7)).float()
        w[:, SIN_UNIT] = 7
        w[:, NEG_UNIT] = 5
        w[:, LABEL_UNIT] = W_LABEL
        new[name + ".mlp.1.weight"], new[name + ".mlp.1.bias"] = w, b
        g0 += 2 * cout
    for k, v in new.items():
        assert sd["model." + k].shape == v.shape, k
        sd["model." + k] = v
    return sd


def designed_trace(sd, dim, log_snr, class_ids) -> float:
    """Every intermediate of the designed table, in float64 with the devices applied, asserted to stay inside the sets the devices
    need: pre-GELU values multiples of 16, pre-SiLU values in {0} u [32, inf) u (-inf, -96], every sum of magnitudes - a bound of
    every partial sum in any order - below 2^24.  Returns the largest such sum."""
    s = {k: v.double() for k, v in strip(sd).items() if k.startswith(("time_mlp", "class_mlp")) or ".mlp.1." in k}
    gelu = lambda v: torch.where(v >= 16, v, torch.zeros_like(v))
    top = 0.0

    def lin(x, w, b):
        nonlocal top
        top = max(top, float((x.abs() @ w.abs().T + b.abs()).max()))
        return x @ w.T + b

    assert not s["time_mlp.0.weights"].any()
    x = torch.tensor(log_snr, dtype=torch.float64)[:, None]
    f = torch.cat((x, torch.zeros(len(log_snr), HALF, dtype=torch.float64), torch.ones(len(log_snr), HALF, dtype=torch.float64)), 1)
    pre = lin(f, s["time_mlp.1.weight"], s["time_mlp.1.bias"])
    assert bool((pre % 16 == 0).all()) and bool((pre >= 16).any()) and bool((pre <= -16).any())
    t = lin(gelu(pre), s["time_mlp.3.weight"], s["time_mlp.3.bias"])
    rows = []
    for i in range(len(log_snr)):
        for k in range(len(class_ids) + 1):
            v = t[i]
            if k < len(class_ids) and class_ids[k] >= 0:
                pc = lin(s["class_mlp.0.weight"][class_ids[k]][None], s["class_mlp.1.weight"], s["class_mlp.1.bias"])
                assert bool((pc % 16 == 0).all())
                v = v + lin(gelu(pc), s["class_mlp.3.weight"], s["class_mlp.3.bias"])[0]
            rows.append(v)
    trows = torch.stack(rows)
    assert bool(((trows == 0) | (trows >= 32) | (trows <= -96)).all()) and bool((trows <= -96).any()) and bool((trows >= 32).any())
    act = torch.where(trows >= 32, trows, torch.zeros_like(trows))
    for name, _ in blocks(dim):
        lin(act, s[name + ".mlp.1.weight"], s[name + ".mlp.1.bias"])
    assert top < 2.0 ** 24, top
    return top


LAYOUT_LOG_SNR = (3.0, 1.0, 4.0, 2.0)                       # small integers, out of order, n = 4
LAYOUT_LABELS = {"K1_label": [1], "K1_no_label": [-1], "K3_out_of_order": [2, 0, 1]}


def designed_code(g, x, label):
    """The integer restatement of one table entry: column code g, log-SNR x, label l (None: no class embedding)."""
    return g + 32 * W_COL * (g % 7) + W_X * 16 * (2 + x) + W_LABEL * 32 * (0 if label is None else label + 1)


def designed_rows(dim, log_snr, class_ids) -> Dict[str, torch.Tensor]:
    """Per block [(K + 1) n, 2 Cout] int64 - the layout comment above compute_conditioning, restated: K + 1 rows per log-SNR value i,
    row i (K + 1) + k with the class embedding of class_ids[k] (none if it is < 0), row i (K + 1) + K without; per block scale | shift."""
    K, n = len(class_ids), len(log_snr)
    out, g0 = {}, 0
    for name, cout in blocks(dim):
        g = torch.arange(g0, g0 + 2 * cout)
        rows = torch.zeros((K + 1) * n, 2 * cout, dtype=torch.int64)
        for i, x in enumerate(log_snr):
            for k in range(K + 1):
                label = class_ids[k] if k < K and class_ids[k] >= 0 else None
                rows[i * (K + 1) + k] = designed_code(g, int(x), label)
        out[name] = rows
        g0 += 2 * cout
    return out


def assemble(rows: Dict[str, torch.Tensor], layout: Dict[str, tuple], ss_stride: int, *, shift_blocks=0) -> torch.Tensor:
    """The table [(K + 1) n, ss_stride] from per-block rows and a layout {block: (ss_offset, Cout)}; ``shift_blocks``: the mutant
    that writes every block at the offset of the block ``shift_blocks`` further on."""
    names = list(layout)
    nrows = next(iter(rows.values())).shape[0]
    table = torch.full((nrows, ss_stride), float("nan"), dtype=torch.float64)
    for j, name in enumerate(names):
        off, cout = layout[names[(j + shift_blocks) % len(names)]]
        w = min(2 * cout, rows[name].shape[1])
        table[:, off:off + w] = rows[name][:, :w].double()
    return table


def default_layout(dim):
    """Blocks back to back in state-dict order - for the CPU tests only; the GPU test takes the layout the engine reports and checks
    that it is a partition of the row."""
    out, off = {}, 0
    for name, cout in blocks(dim):
        out[name] = (off, cout)
        off += 2 * cout
    return out, off


def assert_layout_is_a_partition(layout: Dict[str, tuple], ss_stride: int, dim: int):
    want = dict(blocks(dim))
    assert set(layout) == set(want), (sorted(layout), sorted(want))
    spans = sorted((off, off + 2 * cout) for off, cout in layout.values())
    assert spans[0][0] == 0 and spans[-1][1] == ss_stride and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), spans
    for name, (off, cout) in layout.items():
        assert cout == want[name], (name, cout, want[name])


# ------------------------------------------------------------------------------------------------ 2. the reference of the table
def time_features_ref(w, log_snr, dtype, *, drop_x=False):
    """[x, sin(a), cos(a)] with the argument a = ((x * w) * 2) * pi formed in fp32 in the reference's association - it belongs to
    the model, not to the error - and sin / cos taken in ``dtype``."""
    x = log_snr.float()[:, None]
    a = ((x * w.float()[None, :]) * 2.0) * PI32
    a = a.to(dtype)
    return torch.cat((torch.zeros_like(x).to(dtype) if drop_x else x.to(dtype), a.sin(), a.cos()), dim=-1)


def gelu_tanh(v):
    return F.gelu(v, approximate="tanh")


def table_reference(sd, dim, log_snr, class_ids, dtype, mutant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """Per block [(K + 1) n, 2 Cout] in ``dtype``: oracle.time_embedding, class_embedding and the mlp.1 line of resnet_block, row by
    row as the layout comment has them.  ``mutant`` names a wrong table (MUTANTS)."""
    s = {k: v.to(dtype) for k, v in strip(sd).items() if k.startswith(("time_mlp", "class_mlp")) or ".mlp.1." in k}
    ls = torch.as_tensor(log_snr, dtype=torch.float32)
    K, n = len(class_ids), len(log_snr)
    gelu = gelu_tanh if mutant == "tanh_gelu" else F.gelu
    f = time_features_ref(strip(sd)["time_mlp.0.weights"], ls, dtype, drop_x=mutant == "x_feature_dropped")
    t = F.linear(gelu(F.linear(f, s["time_mlp.1.weight"], s["time_mlp.1.bias"])), s["time_mlp.3.weight"], s["time_mlp.3.bias"])
    if mutant == "off_by_one_time_row":
        t = torch.roll(t, -1, 0)
    emb = []
    for k in range(K):
        l = class_ids[0] if mutant == "class_of_first_label_for_every_k" else class_ids[k]
        if l < 0:
            emb.append(None)
            continue
        e = F.embedding(torch.tensor([l]), s["class_mlp.0.weight"])
        e = F.linear(gelu(F.linear(e, s["class_mlp.1.weight"], s["class_mlp.1.bias"])), s["class_mlp.3.weight"], s["class_mlp.3.bias"])
        emb.append(e[0])
    emb.append(None)
    if mutant == "label_and_null_rows_swapped":
        emb = [emb[-1]] + emb[1:-1] + [emb[0]] if K > 1 else emb[::-1]
    trows = torch.stack([t[i] if emb[k] is None else t[i] + emb[k] for i in range(n) for k in range(K + 1)])
    out = {}
    for name, cout in blocks(dim):
        w, b = s[name + ".mlp.1.weight"], s[name + ".mlp.1.bias"]
        e = F.silu(F.linear(trows, w, b)) if mutant == "silu_after_the_block_linear" else F.linear(F.silu(trows), w, b)
        if mutant == "scale_and_shift_swapped":
            e = torch.cat((e[:, cout:], e[:, :cout]), 1)
        out[name] = e
    return out


MUTANTS = ("off_by_one_time_row", "label_and_null_rows_swapped", "scale_and_shift_swapped", "block_offset_shifted",
           "class_of_first_label_for_every_k", "tanh_gelu", "silu_after_the_block_linear", "x_feature_dropped")


def reference_table(sd, dim, log_snr, class_ids, dtype, layout=None, ss_stride=None, mutant=None) -> torch.Tensor:
    if layout is None:
        layout, ss_stride = default_layout(dim)
    rows = table_reference(sd, dim, log_snr, class_ids, dtype, None if mutant == "block_offset_shifted" else mutant)
    return assemble(rows, layout, ss_stride, shift_blocks=1 if mutant == "block_offset_shifted" else 0)


# ------------------------------------------------------------------------------------------------ 3. values on the random network
def value_log_snr() -> List[float]:
    """0, +-1e-3, the schedule's two ends log_snr_linear(0) = 9.2103 and log_snr_linear(1) = -10.0001, +-20, and the EDM run's own
    c_noise = 0.25 log(sigma) values (oracle.edm_sigmas of the default EdmCfg)."""
    e = O.EdmCfg()
    sig = O.edm_sigmas(e, e.num_sample_steps)[:-1]
    c_noise = [float(O.edm_precond_coeffs(e, s)["c_noise"]) for s in sig[:: max(1, len(sig) // 8)]]
    ends = [float(O.log_snr_linear(torch.tensor(v))) for v in (0.0, 1.0)]
    return [0.0, 1e-3, -1e-3, ends[0], ends[1], 20.0, -20.0] + c_noise


VALUE_LABELS = [2, 0, 1]
VALUE_VARIANTS = ("weights_as_they_are", "sinusoid_weights_x4")


@functools.lru_cache(maxsize=None)
def value_state_dict(dim, variant):
    sd = synth_state_dict(schema(dim), seed=0)
    assert variant in VALUE_VARIANTS
    if variant == "sinusoid_weights_x4":                 # arguments of several hundred radians
        sd["model.time_mlp.0.weights"] = sd["model.time_mlp.0.weights"] * 4
    return sd


@dataclass
class ValueCase:
    log_snr: List[float]
    class_ids: List[int]
    want: Dict[str, torch.Tensor]         # float64 per block
    e32: float
    tol: float
    max_arg: float                        # largest |argument| of sin / cos, radians


@functools.lru_cache(maxsize=None)
def value_case(dim, variant) -> ValueCase:
    sd = value_state_dict(dim, variant)
    ls = value_log_snr()
    want = table_reference(sd, dim, ls, VALUE_LABELS, torch.float64)
    got32 = table_reference(sd, dim, ls, VALUE_LABELS, torch.float32)
    e32 = max(distance(got32[k], want[k]) for k in want)
    top = max(float(v.abs().max()) for v in want.values())
    w = strip(sd)["time_mlp.0.weights"]
    max_arg = float((torch.tensor(ls)[:, None] * w[None, :] * 2 * PI32).abs().max())
    return ValueCase(ls, VALUE_LABELS, want, e32, max(MARGIN * e32, FLOOR_ULPS * ulp32(top)), max_arg)


# ------------------------------------------------------------------------------------------------ 4. the raw launchers
LIN_IN, LIN_OUT, LIN_ROWS = (1, 17, 63, 64, 65, 512), (1, 3, 5, 130), (1, 3)
LIN_ADD = ("none", "one_row", "per_row")            # add = NULL; add_stride = 0; add_stride = out_f + 2
ACT_NONE, ACT_GELU, ACT_SILU_IN = 0, 1, 2
SENTINEL = -777.0


@dataclass
class LinCase:
    x: torch.Tensor            # fp32 [rows, x_stride]: NaN beyond in_f
    W: torch.Tensor            # [out_f, in_f]
    b: Optional[torch.Tensor]  # [out_f]; None for every other case
    add: Optional[torch.Tensor]
    add_stride: int
    x_stride: int
    y_stride: int
    want: torch.Tensor         # fp32 [rows, out_f], exact integers


def _ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


@functools.lru_cache(maxsize=None)
def lin_case(in_f, out_f, rows, add_mode, act) -> LinCase:
    """Integer-exact: act 0 - x in -3..3, W in -2..2; act 1 (GELU on the output) - W and b multiples of 16, so every pre-activation
    is one; act 2 (SiLU on the input) - x in {0, 32..40, -96..-104}.  Strides wider than the rows, NaN in x's padding."""
    gen = torch.Generator().manual_seed(in_f * 1000 + out_f * 10 + rows + 7 * LIN_ADD.index(add_mode) + 31 * act)
    if act == ACT_SILU_IN:
        pick = torch.randint(0, 4, (rows, in_f), generator=gen)
        x = torch.where(pick == 0, torch.zeros(()).double(), torch.where(pick == 1, -96 - _ints(gen, (rows, in_f), 0, 8), 32 + _ints(gen, (rows, in_f), 0, 8)))
    else:
        x = _ints(gen, (rows, in_f), -3, 3)
    W = _ints(gen, (out_f, in_f), -2, 2)
    W[torch.arange(out_f), torch.arange(out_f) % in_f] = 2                 # no all-zero row
    b = (torch.arange(out_f) % 9 - 4).double() if (in_f + out_f) % 2 else None       # distinct neighbours; None for every other shape
    if act == ACT_GELU:
        W, b = W.sign() * 16, None if b is None else b * 16
    xin = torch.where(x >= 32, x, torch.zeros_like(x)) if act == ACT_SILU_IN else x
    if act == ACT_SILU_IN:
        assert bool(((x == 0) | (x >= 32) | (x <= -96)).all())
    s = xin @ W.T + (0 if b is None else b)
    if act == ACT_GELU:
        assert bool((s % 16 == 0).all())
        s = torch.where(s >= 16, s, torch.zeros_like(s))
    add, add_stride = None, 0
    if add_mode == "one_row":
        add = _ints(gen, (1, out_f), -9, 9)
        s = s + add
    elif add_mode == "per_row":
        add_stride = out_f + 2
        add = torch.full((rows, add_stride), float("nan"), dtype=torch.float64)
        add[:, :out_f] = _ints(gen, (rows, out_f), -9, 9)
        s = s + add[:, :out_f]
    assert float(s.abs().max()) < 2.0 ** 24 and float((xin.abs() @ W.abs().T).max()) < 2.0 ** 24
    x_stride, y_stride = in_f + 5, out_f + 3
    xp = torch.full((rows, x_stride), float("nan"), dtype=torch.float64)
    xp[:, :in_f] = x
    f = lambda v: None if v is None else v.float().contiguous()
    return LinCase(f(xp), f(W), f(b), f(add), add_stride, x_stride, y_stride, s.float())


def lin_reference(c: LinCase, in_f, out_f, act, *, mutant=None):
    """float64 linear_rows by its definition; mutants: the bias of the next output, ``add`` of row 0 for every row."""
    x, W = c.x[:, :in_f].double(), c.W.double()
    if act == ACT_SILU_IN:
        x = torch.where(x <= -96, torch.zeros_like(x), x / (1 + torch.exp(-x)))
    s = x @ W.T
    if c.b is not None:
        s = s + (torch.roll(c.b.double(), -1) if mutant == "bias_of_the_next_output" else c.b.double())
    if act == ACT_GELU:
        s = torch.where(s <= -16, torch.zeros_like(s), F.gelu(s))
    if c.add is not None:
        a = c.add[:, :out_f].double()
        s = s + (a[:1] if mutant == "add_of_row_0" or c.add_stride == 0 else a)
    return s


@functools.lru_cache(maxsize=None)
def gelu_sweep():
    """linear_rows' erf-GELU where it is neither the identity nor zero: one row x = [1], W[o] = s_o over 0 and +-2^-10 .. 2 (log-spaced,
    257 per sign), so y[o] = gelu(s_o).  float64 reference; tolerance MARGIN x (F.gelu in fp32 against float64) over the sweep, at
    least 4 ulp of the largest value.  The table tolerances reject the tanh form by a factor of 40 to 70 only - erf- and tanh-GELU
    differ by at most 4.7e-4, 2e-4 of the value, a few hundred fp32 roundings - so it is this case that must reject it by 100."""
    mags = torch.logspace(-10, 1, 257, base=2.0, dtype=torch.float64)       # (beyond 2 torch's own fp32 GELU is 3 ulp off and the bound widens)
    s = torch.cat((torch.zeros(1, dtype=torch.float64), mags, -mags)).float()
    want = F.gelu(s.double())
    e32 = distance(F.gelu(s), want)
    return s, want, max(MARGIN * e32, FLOOR_ULPS * ulp32(float(want.abs().max())))


TF_HALF, TF_ROWS = (1, 8, 64, 65), (1, 3, 5)


@functools.lru_cache(maxsize=None)
def tf_case(half, rows, kind):
    """kind "zero": w = 0, the features are exactly [x, 0.., 1..]; kind "values": w ~ 4 N(0, 1) and x up to +-20 - arguments of several
    hundred radians - against float64 sin / cos of the fp32 argument, tolerance MARGIN x (torch's fp32 sin / cos against float64),
    at least 4 ulp of 1."""
    gen = torch.Generator().manual_seed(half * 10 + rows)
    x = torch.tensor([20.0, -20.0, 9.2103, -10.0001, 1e-3][:rows]) if kind == "values" else torch.arange(1, rows + 1).float() * 3 - 5
    w = 4 * torch.randn(half, generator=gen) if kind == "values" else torch.zeros(half)
    want = time_features_ref(w, x, torch.float64)
    e32 = distance(time_features_ref(w, x, torch.float32), want)
    tol = 0.0 if kind == "zero" else max(MARGIN * e32, FLOOR_ULPS * ulp32(1.0))
    return x, w, want, tol


# ------------------------------------------------------------------------------------------------ 5. gn_finalize's row addressing
GNC_C = ((16, 8), (96, 6), (128, 8))                # (C, groups)
GNC_STEPS = ((None, 2), (0, 2), (1, 2), (7, 2), (1, 8), (7, 8))       # (device step value or None: no step pointer, step_mul)
GNC_ROWS = (3, 0, 4, 1, 2)                          # ss_rows: a permutation, B = 5
GNC_OFFSET, GNC_PAD = 32, 24


def gnc_table(C):
    """Entries encode (row, column): 4096 row + column; rows for every step value and multiplier; exact up to the sum of two."""
    stride = GNC_OFFSET + 2 * C + GNC_PAD
    nrows = max(GNC_ROWS) + 7 * 8 + 1
    r, c = torch.arange(nrows)[:, None], torch.arange(stride)[None, :]
    return (4096 * r + c).float(), stride


def gnc_want(C, beta1: bool, step, step_mul):
    """coefB with gamma = 0: beta = 0 -> shift, beta = 1 -> scale + 1 + shift, of row ss_rows[b] + step * step_mul at ss_offset."""
    table, _ = gnc_table(C)
    rows = torch.tensor(GNC_ROWS) + (0 if step is None else step * step_mul)
    scale = table[rows, GNC_OFFSET:GNC_OFFSET + C].double()
    shift = table[rows, GNC_OFFSET + C:GNC_OFFSET + 2 * C].double()
    want = scale + 1 + shift if beta1 else shift
    assert float(want.max()) < 2.0 ** 24
    return want.float()


# ------------------------------------------------------------------------------------------------ 6. conditioning rows of a sampler step
# launch_step_rows (engine.hip: fill_rows_kernel, fill_rows_labels_kernel).  A run of three equal images, two even-grid tiles and one
# odd-grid tile each: the device tile lists are image-major, so even tiles 0..5 belong to images 0 0 1 1 2 2, odd tiles 0..2 to 0 1 2.
STEP_TILE = 64
STEP_IMAGES = 3
STEP_TILES = {0: [(0, 0), (STEP_TILE, 0)], 1: [(STEP_TILE // 2, 0)]}           # parity -> (y, x) of one image's tiles
STEP_LABEL_MODES = {"one_label": 1, "no_label": -1, "per_image": [2, 0, 2]}       # class id of the run, or one label per image
STEP_BATCHES = {0: [(0, 6), (0, 4), (4, 2), (1, 3)], 1: [(0, 3), (1, 2), (2, 1)]}  # parity -> (first, nt): sub-batches with first > 0


def step_tile_images(parity) -> List[int]:
    return [im for im in range(STEP_IMAGES) for _ in STEP_TILES[parity]]


def label_slots(ids: List[int]):
    """The distinct labels in order of first appearance, and each image's index among them (the run's K label rows)."""
    labels = []
    for v in ids:
        if v not in labels:
            labels.append(v)
    return labels, [labels.index(v) for v in ids]


def step_row_base(K, ev, slot_or_none):
    """base = (K + 1) * ev + (label slot | K: the null row) - the comment in eval_tile_batch; the step's own (K + 1) * evals * step
    is added on the device."""
    return (K + 1) * ev + (K if slot_or_none is None else slot_or_none)


STEP_MUTANTS = ("ev_ignored", "pass1_null_ignored", "first_ignored", "slot_is_the_label_value", "null_row_is_row_1")


def step_rows_want(mode, parity, nb, nt, first, ev, pass1_null, mutant=None) -> torch.Tensor:
    """Rows of batch entries 0 .. nb: entry i is pass i // nt of tile first + i % nt; pass 1 takes the null row under class guidance
    (pass1_null).  One-label run: K = 1, slot 0; no-label run: K = 1, the null row in both passes; per-image labels: the slot of the
    tile's image."""
    images = step_tile_images(parity)
    spec = STEP_LABEL_MODES[mode]
    if mode == "per_image":
        labels, slots = label_slots(spec)
        K = len(labels)
        if mutant == "slot_is_the_label_value":
            slots = list(spec)
    else:
        K, slots = 1, None
    if mutant == "ev_ignored":
        ev = 0
    if mutant == "first_ignored":
        first = 0
    rows = []
    for i in range(nb):
        p, t = i // nt, first + i % nt
        if p == 1 and pass1_null and mutant != "pass1_null_ignored":
            sel = None
        elif slots is not None:
            sel = slots[images[t]]
        else:
            sel = 0 if spec >= 0 else None
        r = step_row_base(K, ev, sel)
        if sel is None and mutant == "null_row_is_row_1":
            r = (K + 1) * ev + 1
        rows.append(r)
    return torch.tensor(rows, dtype=torch.int32)


def step_launches(mode, evals):
    """Every launch of the case set: (parity, nb, nt, first, ev, pass1_null) - one and two passes, with and without the null pass,
    every evaluation of the step (DDPM: evals = 1; EDM: evals = 2, both ev)."""
    out = []
    for parity, batches in STEP_BATCHES.items():
        for first, nt in batches:
            for ev in range(evals):
                out.append((parity, nt, nt, first, ev, 0))
                for null in (0, 1):
                    out.append((parity, 2 * nt, nt, first, ev, null))
    return out
