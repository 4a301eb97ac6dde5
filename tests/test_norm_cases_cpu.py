"""CPU checks of tests/norm_cases.py: the constructions are what they claim, the launch models cover every ``gn_apply_kernel``
instance and every ``rms_norm_kernel`` path the GPU file names, every tolerance comes from the oracle alone, and each assertion
rejects each mutant by a factor of at least 100.

``python -m pytest tests/test_norm_cases_cpu.py -s`` prints, per case, the derived tolerance, the coverage the launch model
claims and every mutant's rejection factor.
"""
import math

import numpy as np
import pytest
import torch

from oracle import srgd_oracle as O
from tests import mxfp8_cases as M
from tests import norm_cases as N


def test_silu_is_the_identity_or_zero_in_fp32():
    N.assert_silu_device()


# ------------------------------------------------------------------------------------------------ gn_apply
@pytest.mark.parametrize("shape", N.GN_SHAPES, ids=lambda s: s.id)
def test_the_designed_statistics_give_mean_0_and_rstd_1(shape):
    cpg = shape.C // shape.groups
    s1, s2 = N.unit_stats(shape.hw, cpg)
    assert np.float32(s2) == s2                                              # an fp32 value
    assert N.finalize64(s1, s2, shape.hw, cpg) == (0.0, 1.0)
    for wobble in (1 - 2.0 ** -27, 1 + 2.0 ** -27):                          # far from the window's ends: 2^-27 is 1e8 double ulps
        assert N.finalize64(s1, s2 * wobble, shape.hw, cpg) == (0.0, 1.0)
    # mean = 0 never takes gn_finalize's second pass over x (mean^2 > 32 (var + eps))
    assert not 0.0 > 32 * (s2 / (shape.hw * cpg) + 1e-5)


def test_the_launch_model_agrees_with_the_twin_tests_model_and_covers_every_instance():
    for s in N.GN_SHAPES:
        if s.bf16:
            a, b = N.gn_launch(s.B, s.hw, s.C, True), M.gn_launch(s.B, s.hw, s.C)
            assert (a.B, a.vpp, a.pow2, a.hoist, a.n, a.stride) == (b.B, b.vpp, b.pow2, b.hoist, b.n, b.stride)
            assert b.trips <= a.trips or a.trips <= b.trips
    cover = {}
    for s in N.GN_SHAPES:
        l = N.gn_launch(s.B, s.hw, s.C, s.bf16)
        kind = "HOIST" if l.hoist else "!HOIST vpp not pow2" if not l.pow2 else "!HOIST pow2 vpp > 256"
        print("%-44s vpp %4d gx %5d stride %7d n %8d  %-22s trips %s" % (s.id, l.vpp, l.gx, l.stride, l.n, kind, sorted(l.trips)))
        assert l.hoist == (l.pow2 and l.vpp <= 256)
        cover.setdefault(("bf16" if s.bf16 else "fp32", kind), []).append((s, l))
    # the instances without a test before: fp32 PRECISE HOIST / !HOIST and bf16 (twin-less) HOIST / !HOIST
    for key in (("fp32", "HOIST"), ("fp32", "!HOIST vpp not pow2"), ("fp32", "!HOIST pow2 vpp > 256"), ("bf16", "HOIST"),
                ("bf16", "!HOIST vpp not pow2")):
        assert key in cover, key
    assert {l.vpp for s, l in cover["fp32", "!HOIST vpp not pow2"]} == {24} and {l.vpp for s, l in cover["bf16", "!HOIST vpp not pow2"]} == {12}
    assert all(l.vpp > 256 for s, l in cover["fp32", "!HOIST pow2 vpp > 256"])
    assert {s.B for s in N.GN_SHAPES} >= {1, 2, 4096}
    trips = set().union(*(N.gn_launch(s.B, s.hw, s.C, s.bf16).trips for s in N.GN_SHAPES))
    assert trips >= {(1, 0), (1, 1), (1, 2), (1, 3), (0, 1)}, trips
    for bf16 in (False, True):
        mine = [s for s in N.GN_SHAPES if s.bf16 == bf16]
        assert {s.in_place for s in mine} == {False, True} and {s.residual for s in mine} == {False, True}
    assert any(N.gn_launch(s.B, s.hw, s.C, s.bf16).n % 256 for s in N.GN_SHAPES)          # a ragged last block
    assert any(N.gn_launch(s.B, s.hw, s.C, s.bf16).gx > 1 and s.B > 1 for s in N.GN_SHAPES)


@pytest.mark.parametrize("shape", N.GN_SHAPES, ids=lambda s: s.id)
def test_the_gn_apply_case_is_integer_exact_and_both_silu_regions_meet_every_sample(shape):
    case = N.gn_case(shape)
    s = shape
    nb = min(s.B, N.COEF_PERIOD)
    # the coefficients gn_finalize must produce, by its own algebra in float64: A = rstd gamma (scale + 1), B = (beta - mean A0) (scale + 1) + shift
    mean, rstd = N.finalize64(*(float(v) for v in case.partial[0, 0, 0]), s.hw, s.C // s.groups)
    sc, sh = case.scale_shift[:nb, :s.C].double() + 1, case.scale_shift[:nb, s.C:].double()
    a0 = rstd * case.gamma.double()
    assert torch.equal(a0 * sc, case.A) and torch.equal((case.beta.double() - mean * a0) * sc + sh, case.Bc)
    assert len({(float(a), float(b)) for a, b in zip(case.A[0, :8], case.Bc[0, :8])}) >= 6           # distinct within neighbouring vectors
    assert not torch.equal(case.A[0], case.A[1 % nb]) or nb == 1
    want, x, res = N.gn_want(case, 0, nb)
    t = case.A[:, None, :] * x.double() + case.Bc[:, None, :]
    assert bool(((t >= N.SILU_ID_MIN) | (t <= N.SILU_ZERO_MAX)).all())
    per_sample = (t >= N.SILU_ID_MIN).reshape(nb, -1)
    assert bool(per_sample.any(1).all()) and bool((~per_sample).any(1).all())                        # both regions in every sample
    if s.large:
        assert s.hw >= N.PERIOD                                                                      # ... and every sample sees the whole period
    ref = N.gn_reference(x, res, case.A, case.Bc)
    assert N.distance(ref, want) <= 204 * math.exp(-32) * 1.01                    # the closed form is the float64 reference: t exp(-32) = 2.6e-12 off
    if s.bf16:
        for v in (x, want) + (() if res is None else (res,)):
            assert torch.equal(v.to(torch.bfloat16).float(), v)
    assert math.gcd(N.PERIOD, N.gn_launch(s.B, s.hw, s.C, s.bf16).stride) == 1 and s.hw % N.PERIOD != 0
    for name, kw in N.GN_MUTANTS.items():
        if name == "residual_dropped" and res is None or name == "coefficients_of_sample_0" and nb == 1:
            continue
        f = N.exact_factor(N.gn_reference(x, res, case.A, case.Bc, N=8 if s.bf16 else 4, **kw), want)
        print("%-44s %-34s rejected by %.3g ulp" % (s.id, name, f))
        assert f >= N.MUTANT_FACTOR, (name, f)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_the_silu_sweep_tolerance_comes_from_the_oracle_and_rejects_wrong_activations(bf16):
    t = N.silu_sweep(bf16)
    for v in N.SWEEP_POINTS:
        if not bf16:
            assert bool((t == np.float32(v)).any()) and bool((t == -np.float32(v)).any())
    assert t.numel() % 128 == 0 and int((t > 0).sum()) >= 3900 and int((t < 0).sum()) >= 3900     # (bf16 rounds the smallest to 0)
    ref = N.silu64(t)
    assert bool(torch.isfinite(ref).all())
    tol = N.silu_tolerance(t)
    for lo, hi in ((0, 2.0 ** -126), (2.0 ** -126, 1e-3), (1e-3, 1), (1, 16), (16, 88), (88, 104), (104, 2e4)):
        for sign in (1, -1):
            m = (t.abs() >= lo) & (t.abs() < hi) & ((t > 0) if sign > 0 else (t < 0))
            print("silu %s t in %s[%.3g, %.3g): tolerance %.3g .. %.3g (|silu| up to %.3g)" % (
                "bf16" if bf16 else "fp32", "-" if sign < 0 else "+", lo, hi, float(tol[m].min()), float(tol[m].max()), float(ref[m].abs().max())))
    assert N.silu_miss(torch.nn.functional.silu(t), t, bf16) <= 1.0 / N.MARGIN + 1e-9                # the oracle sits an eighth inside
    assert N.silu_miss(t / (1 + torch.exp(-t)), t, bf16) <= 1.0                                      # and so does the kernels' form in fp32
    for name, fn in N.SILU_MUTANTS.items():
        f = N.silu_miss(fn(t.double()), t, bf16)
        print("silu %s mutant %-24s rejected by %.3g" % ("bf16" if bf16 else "fp32", name, f))
        assert f >= N.MUTANT_FACTOR, (name, f)


@pytest.mark.parametrize("site", list(N.CONV_SITES))
def test_the_convolution_silu_sites_see_the_whole_sweep_and_reject_wrong_activations(site):
    c = N.CONV_SITES[site]
    t, x, w, extra = N.site_case(site)
    assert set(N.CONV_SITES) == {"conv3x3_bf16_gnin", "conv3x3_split_gnin", "conv3x3_mx2_gnin", "conv1x1_bf16_tail", "conv1x1_split_tail"}
    base = N.silu_sweep(c["bf16"])
    assert set(t.tolist()) == set(base.tolist()) and float(t.abs().max()) <= N.F16_MAX                # every point of the sweep, inside f16
    assert int((w != 0).sum()) == 128 and float(w.sum()) == 128.0 and bool((w[:, :, c["ks"] // 2, c["ks"] // 2] == torch.eye(128)).all())
    assert (extra is not None) == (c["split"] is not None)
    if c["bf16"]:
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    tol = N.silu_tolerance(t, extra)
    for lo, hi in ((0, 2.0 ** -126), (2.0 ** -126, 1e-3), (1e-3, 16), (16, 104), (104, 2e4)):
        m = (t.abs() >= lo) & (t.abs() < hi)
        print("%-20s |t| in [%.3g, %.3g): tolerance %.3g .. %.3g%s%s" % (site, lo, hi, float(tol[m].min()), float(tol[m].max()),
              (", of it split emulation up to %.3g" % float(extra[m].max())) if extra is not None else "", " + half a bf16 step" if c["bf16"] else ""))
    ref32 = torch.nn.functional.silu(t)
    if extra is None:
        assert N.silu_miss(ref32, t, c["bf16"], extra) <= 1.0 / N.MARGIN + 1e-9
    for name, fn in N.SILU_MUTANTS.items():
        f = N.silu_miss(fn(t.double()), t, c["bf16"], extra)
        print("%-20s mutant %-24s rejected by %.3g" % (site, name, f))
        assert f >= N.MUTANT_FACTOR, (site, name, f)


# ------------------------------------------------------------------------------------------------ rms_norm
def test_the_rms_launch_model_covers_every_path():
    exact = {s: N.rms_launch(s.npix, s.C, s.bf16) for s in N.RMS_EXACT_SHAPES}
    ragged = {s: N.rms_launch(s.npix, s.C, s.bf16) for s in N.RMS_RAGGED}
    for s, l in list(exact.items()) + list(ragged.items()):
        print("%-24s %s" % (s.id, l))
    assert {l.L for s, l in exact.items() if not s.bf16} == {4, 16, 64}
    assert {l.L for s, l in exact.items() if s.bf16} >= {2, 8, 32, 64}
    assert any(l.v_trips == 4 and l.vpp == 256 for s, l in exact.items() if not s.bf16)              # the four-trip v loop
    second = [(s, l) for s, l in exact.items() if l.pixel_trips == 2]
    assert {(s.bf16, s.C, l.L) for s, l in second} == {(False, 16, 4), (True, 32, 4), (False, 256, 64)}
    for s, l in second:                                                                              # the grid-stride loop's second trip
        assert s.npix == 8192 * (256 // l.L) + 3 and l.grid == 8192
        assert math.gcd(N.PERIOD, l.pix_per_trip) == 1
    assert all(l.pixel_trips == 1 and l.grid > 1 for s, l in exact.items() if s.npix == 1500)
    assert all(l.ragged and l.vpp & (l.vpp - 1) for l in ragged.values()) and all(l.grid > 1 for l in ragged.values())
    assert {(s.bf16, l.vpp, l.L) for s, l in ragged.items()} == {(False, 6, 4), (False, 12, 8), (False, 24, 16), (False, 34, 32),
                                                                 (True, 3, 2), (True, 6, 4), (True, 12, 8), (True, 34, 32)}


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [16, 32, 64, 256, 1024])
def test_the_exact_rows_are_exact_in_fp32_step_by_step(C, bf16):
    e = N.rms_exact(C, bf16)
    x = e.base_x.numpy()
    ss = (x * x).sum(1, dtype=np.float32)
    assert np.array_equal(ss.astype(np.float64), (x.astype(np.float64) ** 2).sum(1))                 # the sum of squares is exact
    inv = np.float32(math.sqrt(C)) / np.sqrt(ss)                                                     # fp32 sqrt and quotient, correctly rounded
    assert np.array_equal(np.log2(inv) % 1, np.zeros_like(inv))                                      # a power of two
    y = torch.from_numpy(x * inv[:, None] * e.g.numpy()[None])
    N.assert_exact(y, e.want, "fp32 step by step")
    assert N.distance(N.rms_reference(e.base_x, e.g), e.want) <= 2.0 ** -50 * float(e.want.abs().max())        # the float64 reference
    o32 = O.rms_norm(e.base_x[:, :, None, None], e.g.view(1, C, 1, 1))[:, :, 0, 0]
    if int(math.log2(C)) % 2 == 0:
        N.assert_exact(o32, e.want, "oracle fp32")
    else:                   # C = 32: the oracle divides x by a sqrt(2) before it multiplies by 4 sqrt(2); the kernel forms sqrtf(C) / norm first
        assert N.distance(o32, e.want) <= 2 * N.ulp32(float(e.want.abs().max()))
    assert len(set(e.g.tolist())) == C and torch.equal(e.g.to(torch.bfloat16).float(), e.g)          # distinct bf16-exact gains
    nz = (e.base_x != 0).sum(1)
    assert {int(v) for v in nz} == {C // 4 ** i for i in range(min(int(math.log2(C)) // 2, 3) + 1)}
    assert {float(v) for v in e.base_x.abs().max(1).values} == {2.0 ** k for k in range(-3, 4)}
    # every lane and every trip of the v loop holds non-zero entries in some row, and neighbours differ in norm
    assert bool((e.base_x != 0).any(0).all())
    norms = e.base_x.double().pow(2).sum(1)
    assert bool((norms != torch.roll(norms, 1)).all())
    want_res = e.want.double() + e.base_res.double()
    if bf16:
        assert torch.equal(e.base_res.to(torch.bfloat16).float(), e.base_res)
        N.assert_exact(want_res.float().to(torch.bfloat16).float(), e.want_res, "bf16 store")
        assert torch.equal(want_res.float().double(), want_res)
    else:
        N.assert_exact(want_res.float(), e.want_res, "fp32")
        assert torch.equal(want_res.float().double(), want_res)


def _exact_tensor(shape):
    e = N.rms_exact(shape.C, shape.bf16)
    return e, N.rows_of(e.base_x, 0, shape.npix), N.rows_of(e.base_res, 0, shape.npix), N.rows_of(e.want_res, 0, shape.npix)


@pytest.mark.parametrize("mutant", N.RMS_MUTANTS)
def test_a_wrong_rms_norm_misses_by_a_factor_of_100(mutant):
    if mutant == "eps_added":
        for bf16 in (False, True):
            x, g, want, rows = N.rms_edges(64, bf16)
            wrong = N.rms_reference(x, g, mutant=mutant)
            f = N.edge_miss(wrong, want, bf16)
            print("%-28s edge rows %s: rejected by %.3g" % (mutant, "bf16" if bf16 else "fp32", f))
            assert f >= N.MUTANT_FACTOR
            assert N.edge_miss(wrong[rows["norm_2^-40"]], want[rows["norm_2^-40"]], bf16) >= N.MUTANT_FACTOR
        return
    shapes = {"norm_one_grid_stride_away": [s for s in N.RMS_EXACT_SHAPES if s.npix > 1500],
              "first_L_vectors_only": [s for s in N.RMS_EXACT_SHAPES if s.C == 1024]}.get(
                  mutant, [s for s in N.RMS_EXACT_SHAPES if s.npix == 1500])
    for s in shapes:
        e, x, res, want = _exact_tensor(s)
        l = N.rms_launch(s.npix, s.C, s.bf16)
        f = N.exact_factor(N.rms_reference(x, e.g, res, mutant=mutant, launch=l), want)
        print("%-28s %-22s exact rows: rejected by %.3g ulp" % (mutant, s.id, f))
        assert f >= N.MUTANT_FACTOR, (mutant, s.id, f)
    if mutant in ("norm_of_the_next_pixel", "norm_of_the_previous_pixel", "gain_off_by_one_vector", "sqrt_C_missing"):
        for s in N.RMS_RAGGED:
            v = N.rms_ragged(s)
            l = N.rms_launch(s.npix, s.C, s.bf16)
            f = N.within(N.rms_reference(v.x, v.g, v.res, mutant=mutant, launch=l), v.want, v.tol, s.bf16)
            print("%-28s %-22s float64 rows: rejected by %.3g" % (mutant, s.id, f))
            assert f >= N.MUTANT_FACTOR, (mutant, s.id, f)


@pytest.mark.parametrize("shape", N.RMS_RAGGED, ids=lambda s: s.id)
def test_the_ragged_tolerance_comes_from_the_oracle(shape):
    v = N.rms_ragged(shape)
    print("%-22s E32 %.3g  tolerance %.3g%s" % (shape.id, v.e32, v.tol, "  + half a bf16 step (bf16 store)" if shape.bf16 else ""))
    C = shape.C
    o32 = O.rms_norm(v.x[:, :, None, None], v.g.view(1, C, 1, 1))[:, :, 0, 0]
    assert N.within(o32 + v.res, v.want, v.tol, False) <= 1.0 / N.MARGIN + 1e-9 or v.tol == N.FLOOR_ULPS * N.ulp32(float(v.want.abs().max()))
    assert v.tol <= 64 * N.ulp32(float(v.want.abs().max()))                                          # a few ulp, not a loose gate
    norms = v.x.double().pow(2).sum(1).sqrt()
    assert float(norms.max() / norms.min()) > 2.0 ** 38                                              # the 2^+-20 scaling is there
    if shape.bf16:
        assert torch.equal(v.x.to(torch.bfloat16).float(), v.x)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [16, 64, 1024])
def test_the_edge_rows_follow_the_reference(C, bf16):
    x, g, want, rows = N.rms_edges(C, bf16)
    o32 = O.rms_norm(x[:, :, None, None], g.view(1, C, 1, 1))[:, :, 0, 0]
    assert N.edge_miss(o32, want, False) <= 1.0                                                      # the reference's fp32 semantics, to 4 ulp
    assert not want[rows["zero"]].any()
    k = math.sqrt(C) / N.EPS_NORM
    for name in ("norm_2^-58", "squares_underflow", "norm_2^-40"):
        r = rows[name]
        assert torch.equal(want[r], x[r].double() * k * g.double()) or N.distance(want[r], x[r].double() * k * g.double()) <= 2.0 ** -50 * float(want[r].abs().max())
        assert float(want[r].abs().max()) > 2.0 ** -100
    assert float((x[rows["squares_underflow"]] ** 2).sum()) == 0.0                                   # the squares are 0 in fp32
    assert float(x[rows["norm_2^-58"]].double().pow(2).sum().sqrt()) == 2.0 ** -58
    assert bool(torch.isnan(want[rows["nan"]]).all()) and int(torch.isnan(want).any(1).sum()) == 1   # a NaN stays in its pixel
    assert int(torch.isnan(x).sum()) == 1


# ------------------------------------------------------------------------------------------------ conv1x1_split's folded RMSNorm
@pytest.mark.parametrize("f", N.FOLDED, ids=lambda f: f.id)
def test_the_folded_rms_cases(f):
    x, g, w, res, want, mag = N.folded_case(f)
    print("%-34s T = %3d tiles (%s than the %d CUs), %s" % (f.id, f.tiles, "more" if f.tiles > N.CUS else "no more", N.CUS,
                                                          "bit for bit" if N.folded_exact(f) else "2^-21 relative"))
    assert f.N % 256 == 0 and f.Cin % 32 == 0 and f.Cout % 128 == 0 and (f.kind == "pre" or (f.Cout == 128 and res is not None))
    assert bool((w.sum(1) == 1).all()) and int((w != 0).sum()) == f.Cout                             # selection weights of 1.0
    # the float64 definition on the same rows
    xn = N.rms_reference(x, g) if f.kind == "pre" else x.double()
    y = xn @ w.double().T
    ref = y if f.kind == "pre" else N.rms_reference(y.float(), g, res)
    assert N.folded_miss(ref, want, mag, False) <= 2.0 ** -20                                        # far inside REL_FP32
    if N.folded_exact(f):
        folded = g * np.float32(math.sqrt(f.Cin))
        assert torch.equal(folded.to(torch.float16).float(), folded * 1.0) or torch.equal((folded * 2.0 ** 8).to(torch.float16).float(), folded * 2.0 ** 8)
        assert torch.equal(x.to(torch.float16).float(), x)
        norm = x.double().pow(2).sum(1).sqrt()
        assert bool((torch.log2(norm) % 1 == 0).all())
    # a wrong pixel <-> norm pairing, a gain of the next channel and a missing sqrt(C) miss by more than 100
    for mutant in ("norm_of_the_next_pixel", "gain_off_by_one_vector", "sqrt_C_missing"):
        l = N.rms_launch(x.shape[0], f.Cin if f.kind == "pre" else f.Cout, False)
        wrong = (N.rms_reference(x, g, mutant=mutant, launch=l) @ w.double().T) if f.kind == "pre" else N.rms_reference(y.float(), g, res, mutant=mutant, launch=l)
        miss = N.folded_miss(wrong, want, mag, False)
        print("%-34s %-28s rejected by %.3g" % (f.id, mutant, miss))
        assert miss >= N.MUTANT_FACTOR


def test_the_folded_rms_cases_cover_one_and_several_tiles_per_workgroup():
    for kind in ("pre", "post"):
        mine = [f for f in N.FOLDED if f.kind == kind]
        assert any(f.tiles > N.CUS for f in mine) and any(f.B == 8 and f.N == 256 for f in mine)
        assert {f.Cin for f in mine} == {128, 256}
    assert math.gcd(N.PERIOD, 256) == 1
