"""Proves the cases of tests/linattn_block_cases.py on the CPU, before tests/test_linattn_block_exact_gpu.py feeds them to the
fused LinearAttention kernels:

  (a) the inputs are exact in bf16 and the host's gain fold is too; the closed forms hold in float64; the scripted maxima of the
      lazy family are reached; the CPU emulation of the kernels and the fp32 oracle stay inside every gate, and the gates are what
      the module says they are - twice the emulation's worst error against float64 (or a floor from the number formats);
  (b) each of the thirteen mutants of the emulation is rejected, at C = 128 and at C = 256, with its worst element >= 4 gates;
  (c) every family rejects at least one mutant.

The tables (emulation error, gate, rejection ratio of every mutant) are printed: run with -s or -rP to see them."""
import math

import pytest
import torch

from tests import linattn_block_cases as LC

CS = (128, 256)
MUTANT_SHAPES = (192, 320, 2112)           # one strip; a ragged strip of 256; a ragged strip of 512 after four whole ones
_RUNS = {}


def run(family, C, N):
    """(case, float64 expectations, emulation), computed once per case."""
    key = (family, C, N)
    if key not in _RUNS:
        case = LC.make_case(family, C, N)
        _RUNS[key] = (case, LC.expected(case), LC.emulate(case))
    return _RUNS[key]


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("family", LC.FAMILIES)
def test_inputs_are_bf16_exact_and_the_fold_is_representable(family, C):
    for N in (64, 320):
        case = LC.make_case(family, C, N)
        P = case["P"]
        for name, t in (("x", case["x"]), ("to_qkv", P["wqkv"]), ("to_out", P["wout"]), ("bias", P["bout"])):
            assert torch.equal(t, LC.bf(t)), name
        assert P["g1"].dtype == torch.float32 and P["g2"].dtype == torch.float32
        # the fold W * (g * sqrt(C)), done in fp32 as the host does it, lands on W * 2^j: bf16 loses nothing, and the float64
        # reference (which multiplies by g * sqrt(C) itself) sees the same weights to 2^-23
        gs = P["g1"].double() * math.sqrt(C)
        j = torch.log2(gs).round()
        assert float((gs / 2.0 ** j - 1).abs().max()) < 2.0 ** -22
        assert torch.equal(LC.folded(P), P["wqkv"] * 2.0 ** j[None, :])
        assert LC.design_strip(N) % LC.tile_px(C) == 0 and N % 64 == 0


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("family", LC.FAMILIES)
def test_written_out_reference_is_the_oracle(family, C):
    for N in (64, 320, 2112):
        case, want, _ = run(family, C, N)
        r = LC.reference(case["x"], case["P"])
        assert float((r["y"] - want["y"]).abs().max()) <= 1e-12 * float(want["y"].abs().max())


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("N", (64, 192, 320, 2112))
def test_count_closed_form(N, C):
    case, want, _ = run("count", C, N)
    r = LC.reference(case["x"], case["P"])
    mean_v = r["v"].mean(0)                                                   # [4][32 e]
    assert float((want["ctxn"] - LC.SCALE * mean_v[:, None, :]).abs().max()) <= 1e-14
    d = want["y"] - case["x"]
    assert float((d - d[:1]).abs().max()) <= 1e-12                            # the attention output is the same for every pixel
    # the bias is of the order of the attention output: a uniform scale error survives RMSNorm2
    ratio = float(case["P"]["bout"].abs().mean() / r["o_nobias"].abs().mean())
    assert 0.25 <= ratio <= 4.0, ratio
    # tiles and strips carry their own weight in the mean: no two tile sums of v agree
    TM = LC.tile_px(C)
    sums = r["v"].reshape(N // TM, TM, 128).sum(1)
    if N // TM > 1:
        assert float(torch.cdist(sums, sums).add(torch.eye(N // TM) * 1e9).min()) > 1e-3


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("N", (64, 128, 320, 2112))
def test_select_closed_form(N, C):
    case, want, _ = run("select", C, N)
    r = LC.reference(case["x"], case["P"])
    k = r["k_log2"]
    top2 = k.topk(2, dim=0).values
    assert float((top2[0] - top2[1]).min()) > 150.0                          # exp2 of the runner-up is 0 in fp32
    sel = torch.tensor([[LC.select_position(N, h, d) for d in range(32)] for h in range(4)])
    assert torch.equal(k.argmax(0), sel)
    if N >= 128:
        assert len(set(sel.reshape(-1).tolist())) == 128                      # a position of its own per head and per d
        TM = LC.tile_px(C)
        tiles = set((sel // TM).reshape(-1).tolist())
        assert 0 in tiles and N // TM - 1 in tiles
    ctx_cf = torch.stack([r["v"][sel[h], h, :] for h in range(4)]) * LC.SCALE    # the context is one v row
    assert float((want["ctxn"] - ctx_cf).abs().max()) <= 1e-14
    # the output pairs them through q (the pixels without a runner-up)
    n = torch.arange(N)
    hard = n[n % 4 != 2]
    P = case["P"]
    att = torch.cat([ctx_cf[h][torch.tensor([LC.select_q(int(i), h) for i in hard])] for h in range(4)], dim=1)
    o = att @ P["wout"].T + P["bout"]
    y = o / o.norm(dim=1, keepdim=True) * P["g2"].double() * math.sqrt(C) + case["x"][hard]
    assert float((want["y"][hard] - y).abs().max()) <= 1e-12


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("N", (128, 192, 320, 2112, 16576))
def test_lazy_script_is_reached(N, C):
    case, _, emu = run("lazy", C, N)
    TM, strip = LC.tile_px(C), LC.design_strip(N)
    tps = strip // TM
    cls = torch.arange(32) % 4
    seen = set()
    for tr in emu["trace"]:
        t, rise, f = tr["tile"], tr["rise"], tr["f"]
        ti, s = t % tps, t // tps
        T = min(tps, N // TM - s * tps)
        last_ragged = t == N // TM - 1 and T < tps and ti >= 2
        if ti == 1 or last_ragged:
            where = "second" if ti == 1 else "last_ragged"
            # head 0: under 8 (the reference point holds, p reaches ~2^8), over 8, 40 or more, a fall of 30 or more
            assert bool(((rise[0][cls == 0] > 7.0) & (rise[0][cls == 0] < 8.0)).all()) and bool((f[0][cls == 0] == 1).all())
            assert bool(((rise[0][cls == 1] > 8.0) & (rise[0][cls == 1] < 9.0)).all()) and bool((f[0][cls == 1] < 1).all())
            assert bool((rise[0][cls == 2] >= 40.0).all())
            if s % 2 == 0 and ti == 1:
                assert bool((rise[0][cls == 3] <= -30.0).all()) and bool((f[0][cls == 3] == 1).all())
            # head 1: 32 distinct jumps over 8 in one tile - 32 different rescale factors, in both lane halves
            assert bool((rise[1] > 8.0).all()) and len(set(f[1].tolist())) == 32 and bool((f[1] < 2.0 ** -8).all())
            assert bool((f[2:] == 1).all())                                   # heads 2 and 3 hold still
            seen.add(where)
        if ti == 0 and s >= 1:
            seen.add("first_of_later_strip")
    assert "second" in seen
    if N > strip:
        assert "first_of_later_strip" in seen
        # the strips' reference points differ (the combine path has work to do), by every class of step
        K = LC.lazy_script(C, N)
        d01 = K[tps, 0] - K[0, 0]
        assert bool((d01[cls == 0] > 7).all() and (d01[cls == 1] > 8).all() and (d01[cls == 2] >= 40).all() and (d01[cls == 3] <= -30).all())
    if N % strip and (N % strip) // TM >= 3:
        assert "last_ragged" in seen


@pytest.mark.parametrize("C", CS)
def test_gaussian_spike_moves_the_reference_point_on_live_data(C):
    for N in (192, 320, 2112):
        _, _, emu = run("gaussian", C, N)
        late = [t for t in emu["trace"] if not t["first"] and bool((t["f"] < 1).any())]
        assert late, "no rescale after the first tile of a strip"


def _fit(family, C):
    ew = {t: [] for t in LC.TENSORS}
    for N in LC.SHAPES_CPU:
        _, want, emu = run(family, C, N)
        for t in LC.TENSORS:
            ew[t].append(((emu[t] - want[t]).abs(), want[t]))
    return {t: LC.fit_gate(ew[t], t, C) for t in LC.TENSORS}, ew


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("family", LC.FAMILIES)
def test_emulation_and_fp32_oracle_stay_inside_every_gate(family, C):
    fitted, ew = _fit(family, C)
    for t in LC.TENSORS:
        a, b = LC.GATES[(family, C, t)]
        fa, fb = fitted[t]
        emax = max(float(e.max()) for e, _ in ew[t])
        wmax = max(float(w.abs().max()) for _, w in ew[t])
        print(f"linattn block gates {family:9s} C={C} {t:5s}: emulation max|err| {emax:.4g} (max|want| {wmax:.4g}); "
              f"fitted a={fa:.4g} b={fb:.4g}; gate a={a:g} b={b:g}")
        # the gate in the module is the fitted one, rounded up (at most 10 %), never fitted to anything else
        assert fa <= a * 1.02 and a <= fa * 1.12, (t, a, fa)
        assert fb <= b * 1.02 + 1e-30 and b <= fb * 1.12, (t, b, fb)
        a_min, _ = LC.gate_floor(t, C)
        assert a >= a_min
    for N in LC.SHAPES_CPU:
        case, want, emu = run(family, C, N)
        r32 = LC.reference(case["x"], case["P"], torch.float32)
        o32 = {"y": LC.oracle_y(case["x"], case["P"], torch.float32), "ctxn": r32["ctxn"], "rinv": r32["rinv"]}
        for t in LC.TENSORS:
            ex_e, _ = LC.excess(emu[t], want[t], family, C, t)
            ex_o, _ = LC.excess(o32[t], want[t], family, C, t)
            assert ex_e <= 0.55, (N, t, ex_e)                                 # the gate is twice the emulation's worst error
            assert ex_o <= 1.0, (N, t, ex_o)


_REJECT = {}


def rejection(C):
    """mutant -> family -> worst element / gate, the largest over MUTANT_SHAPES and the checked tensors."""
    if C not in _REJECT:
        tab = {m: {f: 0.0 for f in LC.FAMILIES} for m in LC.MUTANTS}
        for family in LC.FAMILIES:
            for N in MUTANT_SHAPES:
                case, want, _ = run(family, C, N)
                for m in LC.MUTANTS:
                    emu = LC.emulate(case, m)
                    tab[m][family] = max([tab[m][family]] + [LC.excess(emu[t], want[t], family, C, t)[0] for t in LC.TENSORS])
        _REJECT[C] = tab
        print(f"linattn block mutants, C={C}: worst element / gate per family (N in {MUTANT_SHAPES})")
        print(" " * 28 + "".join(f"{f:>12s}" for f in LC.FAMILIES))
        for m in LC.MUTANTS:
            print(f"{m:28s}" + "".join(f"{tab[m][f]:12.3g}" for f in LC.FAMILIES))
    return _REJECT[C]


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("mutant", LC.MUTANTS)
def test_every_mutant_is_rejected(mutant, C):
    tab = rejection(C)
    assert max(tab[mutant].values()) >= 4.0, tab[mutant]


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("family", LC.FAMILIES)
def test_no_family_is_vacuous(family, C):
    tab = rejection(C)
    caught = [m for m in LC.MUTANTS if tab[m][family] >= 4.0]
    assert caught, family
    # and the unmutated emulation passes the same cases
    for N in MUTANT_SHAPES:
        _, want, emu = run(family, C, N)
        assert all(LC.excess(emu[t], want[t], family, C, t)[0] <= 1.0 for t in LC.TENSORS)
