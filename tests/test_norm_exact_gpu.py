"""``gn_apply_kernel`` (every instance without the MX-fp8 twin) and ``rms_norm_kernel`` of srgd_amd/csrc/norm_act.hip against the
closed forms and float64 references of tests/norm_cases.py, through srgd_k_groupnorm_silu and srgd_k_rmsnorm.

gn_apply, index-exact (bit for bit, -0 == +0): designed statistics make gn_finalize hand over mean 0 and rstd 1, so the
coefficients are the small integers gamma (scale + 1) and beta (scale + 1) + shift; every pre-activation is >= 32 (SiLU is the
identity) or <= -96 (SiLU is zero).  Shapes by the launch model: fp32 PRECISE with HOIST (C / 4 = 4, 32), without it at 24 vectors
per pixel (C = 96) and at 512 (C = 2048); bf16 with HOIST (4, 16) and without (12); B = 1, 2, 4096; one four-vector trip followed
by 0 | 1 (fp32, 4124 vectors per sample) and 2 | 3 (bf16, 6172) single trips; in place and out of place, with and without
residual; guard bands on both sides of the output.

SiLU over its whole range through gn_apply (A = 1, B = 0), fp32 (expf) and bf16 (__expf + rcp): +-{0, 2^-130, ..., 88.7, 89, ...,
104, 1e4} and 4096 log-spaced magnitudes, where exp(-t) overflows and where 1 + exp(-t) rounds to 1; finite wherever the
reference is.  The same sweep at the convolutions' SiLU sites (norm_cases.CONV_SITES): GroupNorm in staging of conv3x3_bf16 (impl 5),
conv3x3_split (11) and the conv3x3_mx2 prototype (15) behind centre-tap selection weights, and the GroupNorm-tail epilogues of
conv1x1_bf16 (3) and conv1x1_split (10) with x = 0; the split sites are granted the split emulation's distance per binade.

rms_norm: the bit-exact rows (pixel <-> norm pairing, gain index, L = 4, 16, 64 and the four-trip v loop at C / N = 256) with
residual out of place and without residual in place; the same rows over the grid-stride loop's SECOND TRIP (8192 * 256 / L + 3
pixels: fp32 C = 16 and bf16 C = 32 at L = 4, fp32 C = 256 at L = 64); ragged C / N against float64; the edge rows (zero row,
norm 2^-58 and 2^-40 under the clamp, squares that underflow, a NaN that stays in its pixel); the RMSNorm folded into
conv1x1_split (srgd_k_conv1x1_split_rms) on the same rows with selection weights: pre-norm Cin 128 / 256 -> Cout 384, post-norm
Cout 128 with residual, one tile per workgroup (B = 8, N = 256) and several (T = 288 / 320 tiles over 256 CUs) - bit for bit where
every intermediate is exact (pre-norm, Cin = 256), 2^-21 relative otherwise.

A bf16 tensor's storage rounding is granted as half a bf16 step at the reference's own bf16 rounding (norm_cases.bf16_store_bound): 2^-9 of the value
at the top of a binade, 2^-8 at the bottom.  2^-9 of the value everywhere cannot hold for a correctly rounded store: under it the
bf16 SiLU sweep measured 1.96 x the bound at t = 0.015564, where the kernel stores 2^-7, the bf16 nearest to silu64(t) = 0.00784254.

Measured on an MI355X (tolerances: from the oracle alone, tests/test_norm_cases_cpu.py -s prints them; "GPU": measured):

    gn_apply index-exact  fp32_B1_hw67_C16                         HOIST  vpp   4 trips [[0, 1]]           mismatches 0 of 1072
    gn_apply index-exact  fp32_B2_hw131_C128_res                   HOIST  vpp  32 trips [[0, 1]]           mismatches 0 of 33536
    gn_apply index-exact  fp32_B2_hw67_C96_inplace_res             !HOIST vpp  24 trips [[0, 1]]           mismatches 0 of 12864
    gn_apply index-exact  fp32_B1_hw5_C2048_inplace                !HOIST vpp 512 trips [[0, 1]]           mismatches 0 of 10240
    gn_apply index-exact  fp32_B4096_hw1031_C16_inplace_res        HOIST  vpp   4 trips [[1, 0], [1, 1]]   mismatches 0 of 67567616
    gn_apply index-exact  bf16_B1_hw67_C32_inplace                 HOIST  vpp   4 trips [[0, 1]]           mismatches 0 of 2144
    gn_apply index-exact  bf16_B2_hw131_C128_res                   HOIST  vpp  16 trips [[0, 1]]           mismatches 0 of 33536
    gn_apply index-exact  bf16_B2_hw67_C96                         !HOIST vpp  12 trips [[0, 1]]           mismatches 0 of 12864
    gn_apply index-exact  bf16_B2_hw67_C96_inplace_res             !HOIST vpp  12 trips [[0, 1]]           mismatches 0 of 12864
    gn_apply index-exact  bf16_B4096_hw1543_C32_res                HOIST  vpp   4 trips [[1, 2], [1, 3]]   mismatches 0 of 202244096
    gn_apply SiLU range   fp32  worst |err| / tolerance 0.189 (at t = 0.000171106: |err| 7.56e-12, tolerance 4e-11)
    gn_apply SiLU range   bf16  worst |err| / tolerance 1 (at t = 9.18355e-41: |err| 4.59e-41, tolerance 4.59e-41)
    conv SiLU site range  conv3x3_bf16_gnin    impl  5 worst |err| / tolerance 1 (at t = 9.18355e-41: |err| 4.59e-41, tolerance 4.59e-41)
    conv SiLU site range  conv3x3_split_gnin   impl 11 worst |err| / tolerance 1 (at t = 5.87632e-08: |err| 2.94e-08, tolerance 2.94e-08)
    conv SiLU site range  conv3x3_mx2_gnin     impl 15 worst |err| / tolerance 1 (at t = 2.90699e-08: |err| 1.45e-08, tolerance 1.45e-08)
    conv SiLU site range  conv1x1_bf16_tail    impl  3 worst |err| / tolerance 1 (at t = 9.18355e-41: |err| 4.59e-41, tolerance 4.59e-41)
    conv SiLU site range  conv1x1_split_tail   impl 10 worst |err| / tolerance 0.189 (at t = 0.000171106: |err| 7.56e-12, tolerance 4e-11)
    rms_norm exact rows   fp32_C16_npix1500      L  4 v-trips 1 pixel-trips 1  mismatches 0 (residual) 0 (in place) of 24000
    rms_norm exact rows   fp32_C64_npix1500      L 16 v-trips 1 pixel-trips 1  mismatches 0 (residual) 0 (in place) of 96000
    rms_norm exact rows   fp32_C256_npix1500     L 64 v-trips 1 pixel-trips 1  mismatches 0 (residual) 0 (in place) of 384000
    rms_norm exact rows   fp32_C1024_npix1500    L 64 v-trips 4 pixel-trips 1  mismatches 0 (residual) 0 (in place) of 1536000
    rms_norm exact rows   bf16_C16_npix1500      L  2 v-trips 1 pixel-trips 1  mismatches 0 (residual) 0 (in place) of 24000
    rms_norm exact rows   bf16_C64_npix1500      L  8 v-trips 1 pixel-trips 1  mismatches 0 (residual) 0 (in place) of 96000
    rms_norm exact rows   bf16_C256_npix1500     L 32 v-trips 1 pixel-trips 1  mismatches 0 (residual) 0 (in place) of 384000
    rms_norm exact rows   bf16_C1024_npix1500    L 64 v-trips 2 pixel-trips 1  mismatches 0 (residual) 0 (in place) of 1536000
    rms_norm exact rows   fp32_C16_npix524291    L  4 v-trips 1 pixel-trips 2  mismatches 0 (residual) 0 (in place) of 8388656
    rms_norm exact rows   bf16_C32_npix524291    L  4 v-trips 1 pixel-trips 2  mismatches 0 (residual) 0 (in place) of 16777312
    rms_norm exact rows   fp32_C256_npix32771    L 64 v-trips 1 pixel-trips 2  mismatches 0 (residual) 0 (in place) of 8389376
    rms_norm ragged       fp32_C24_npix131       E32 5.13e-07 tolerance 4.11e-06 GPU 6.76e-07 (residual) 6.16e-07 (in place)  worst / bound 0.165
    rms_norm ragged       fp32_C48_npix131       E32 4.96e-07 tolerance 3.97e-06 GPU 3.53e-07 (residual) 3.84e-07 (in place)  worst / bound 0.0889
    rms_norm ragged       fp32_C96_npix131       E32 7.77e-07 tolerance 6.21e-06 GPU 4.86e-07 (residual) 5.18e-07 (in place)  worst / bound 0.0783
    rms_norm ragged       fp32_C136_npix131      E32 5.53e-07 tolerance 4.42e-06 GPU 5.53e-07 (residual) 5.16e-07 (in place)  worst / bound 0.125
    rms_norm ragged       bf16_C24_npix131       E32 4.03e-07 tolerance 3.22e-06 GPU 1.35e-02 (residual) 7.40e-03 (in place)  worst / bound 0.999
    rms_norm ragged       bf16_C48_npix131       E32 5.32e-07 tolerance 4.26e-06 GPU 1.56e-02 (residual) 7.81e-03 (in place)  worst / bound 0.999
    rms_norm ragged       bf16_C96_npix131       E32 5.65e-07 tolerance 4.52e-06 GPU 1.56e-02 (residual) 8.77e-03 (in place)  worst / bound 0.999
    rms_norm ragged       bf16_C272_npix131      E32 5.92e-07 tolerance 4.74e-06 GPU 1.56e-02 (residual) 1.32e-02 (in place)  worst / bound 0.999
    rms_norm edge rows    fp32_C16   worst |err| / (4 ulp): zero 0, norm_2^-58 0.11, squares_underflow 0.15, norm_2^-40 0.11, nan 0, plain 0.16
    rms_norm edge rows    bf16_C16   worst |err| / (4 ulp + store): zero 0, norm_2^-58 0.77, squares_underflow 0.94, norm_2^-40 0.77, nan 0, plain 0.93
    rms_norm edge rows    fp32_C64   worst |err| / (4 ulp): zero 0, norm_2^-58 0.051, squares_underflow 0.15, norm_2^-40 0.14, nan 0, plain 0.4
    rms_norm edge rows    bf16_C64   worst |err| / (4 ulp + store): zero 0, norm_2^-58 0.96, squares_underflow 0.97, norm_2^-40 0.96, nan 0, plain 0.98
    rms_norm edge rows    fp32_C1024 worst |err| / (4 ulp): zero 0, norm_2^-58 0.12, squares_underflow 0.15, norm_2^-40 0.1, nan 0, plain 0.38
    rms_norm edge rows    bf16_C1024 worst |err| / (4 ulp + store): zero 0, norm_2^-58 0.7, squares_underflow 0.97, norm_2^-40 0.94, nan 0, plain 1
    folded rms            pre_Cin128_Cout384_B8_N256       T  24  2^-21 relative  |err| / (2^-21 mag) 0.335
    folded rms            pre_Cin256_Cout384_B8_N256       T  24  mismatches 0  |err| / (2^-21 mag) 0
    folded rms            pre_Cin256_Cout384_B2_N12288     T 288  mismatches 0  |err| / (2^-21 mag) 0
    folded rms            post_Cin128_Cout128_B8_N256      T   8  2^-21 relative  |err| / (2^-21 mag) 0.241
    folded rms            post_Cin256_Cout128_B8_N256      T   8  2^-21 relative  |err| / (2^-21 mag) 0.241
    folded rms            post_Cin128_Cout128_B2_N40960    T 320  2^-21 relative  |err| / (2^-21 mag) 0.241

Every distance is reported through test_engine_gpu._report.
"""
import pytest
import torch

from tests import norm_cases as N
from tests.test_engine_gpu import _report
from tests.test_kernels_gpu import DEV, L, ptr, stream

pytestmark = pytest.mark.gpu

SENTINEL = -77.0


def guarded(n, dtype):
    """[GUARD | n | GUARD] elements of ``dtype`` on the device, all SENTINEL; the middle view is 16-byte aligned."""
    buf = torch.full((n + 2 * N.GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[N.GUARD:N.GUARD + n]


def tiled(base, rows, dtype):
    """Row r of the result is base[r % len(base)] (the tiling is done on the device: the data is the CPU's closed form)."""
    return base.to(DEV)[rows % base.shape[0]].to(dtype)


def check_guards(buf, n, what=""):
    N.assert_guards(torch.cat((buf[:N.GUARD], buf[N.GUARD + n:])).float().cpu(), 0, SENTINEL, what)


def mismatches(got, want):
    return int((got.float() != want).sum())


# ------------------------------------------------------------------------------------------------ gn_apply
def groupnorm_silu(x_mid, y_mid, res, partial, B, hw, C, groups, gamma, beta, ss, bf16):
    L().check(L().lib().srgd_k_groupnorm_silu(ptr(x_mid), ptr(y_mid), ptr(res), ptr(partial), B, hw, C, groups, ptr(gamma), ptr(beta),
                                              ptr(ss), 1, int(bf16), stream()), "groupnorm_silu")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", N.GN_SHAPES, ids=lambda s: s.id)
def test_gn_apply_is_index_exact(shape):
    s = shape
    case = N.gn_case(s)
    dtype = torch.bfloat16 if s.bf16 else torch.float32
    n = s.B * s.hw * s.C
    r = torch.arange(s.B * s.hw, device=DEV)
    x = tiled(case.base_x, r, dtype)
    res = None if case.base_res is None else tiled(case.base_res, r, dtype)
    want = case.want_table.to(DEV)[(r // s.hw) % case.want_table.shape[0], r % N.PERIOD]
    buf, mid = guarded(n, dtype)
    if s.in_place:
        mid.copy_(x.reshape(-1))
        x_mid = mid
    else:
        x_mid = x
    partial, gamma, beta, ss = case.partial.to(DEV), case.gamma.to(DEV), case.beta.to(DEV), case.scale_shift.to(DEV)
    groupnorm_silu(x_mid, mid, res, partial, s.B, s.hw, s.C, s.groups, gamma, beta, ss, s.bf16)
    bad = mismatches(mid.reshape(s.B * s.hw, s.C), want)
    launch = N.gn_launch(s.B, s.hw, s.C, s.bf16)
    _report(test="gn_apply_index_exact", case=s.id, mismatches=bad, elements=n, hoist=launch.hoist, vpp=launch.vpp,
            trips=sorted(launch.trips))
    check_guards(buf, n, s.id)
    if bad:
        N.assert_exact(mid.reshape(s.B, s.hw, s.C)[:1].float().cpu(), want.reshape(s.B, s.hw, s.C)[:1].cpu(), s.id + " (sample 0)")
    assert bad == 0, (s.id, bad)
    if not s.in_place:
        assert mismatches(x, tiled(case.base_x, r, torch.float32)) == 0, "input written"


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_gn_apply_silu_over_its_whole_range(bf16):
    t = N.silu_sweep(bf16)
    C, groups = 128, 8
    hw = t.numel() // C
    dtype = torch.bfloat16 if bf16 else torch.float32
    x = t.to(DEV).to(dtype)
    assert torch.equal(x.float().cpu(), t)
    buf, mid = guarded(t.numel(), dtype)
    s1, s2 = N.unit_stats(hw, C // groups)
    partial = torch.tensor([s1, s2], dtype=torch.float32).expand(1, groups, 1, 2).contiguous().to(DEV)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    groupnorm_silu(x, mid, None, partial, 1, hw, C, groups, gamma, beta, None, bf16)
    got = mid.float().cpu()
    miss = N.silu_miss(got, t, bf16)
    err = (got.double() - N.silu64(t)).abs()
    tol = N.silu_tolerance(t) + (N.bf16_store_bound(N.silu64(t)) if bf16 else 0)
    worst = int((err / tol).argmax())
    _report(test="gn_apply_silu_range", case="bf16" if bf16 else "fp32", miss=miss, worst_t=float(t[worst]), worst_err=float(err[worst]),
            worst_tol=float(tol[worst]))
    check_guards(buf, t.numel())
    assert bool(torch.isfinite(got).all())
    assert miss <= 1.0, (miss, float(t[worst]), float(got[worst]), float(N.silu64(t)[worst]))


@pytest.mark.parametrize("site", list(N.CONV_SITES))
def test_convolution_silu_sites_over_the_whole_range(site):
    from tests.test_kernels_gpu import run_conv
    c = N.CONV_SITES[site]
    t, x, w, extra = N.site_case(site)
    B, C = x.shape[0], x.shape[1]
    ones, zeros = torch.ones(B, C), torch.zeros(B, C)
    if c["kind"] == "gnin":                                  # conv(silu(1 * x + 0)), centre tap 1.0; scale and shift in one allocation
        coef = torch.stack([ones, zeros]).contiguous().to(DEV)
        got, _ = run_conv(x, None, w, None, ks=3, stride=1, pad=1, kind=0, bf16=c["bf16"], impl=c["impl"], gn_tail=(None, coef[0], coef[1]))
    else:                                                    # silu(1 * h + 0) + conv(0)
        got, _ = run_conv(torch.zeros_like(x), None, w, None, ks=1, stride=1, pad=0, kind=0, bf16=c["bf16"], impl=c["impl"], gn_tail=(x, ones, zeros))
    got = got.reshape(-1)
    tol = N.silu_tolerance(t, extra) + (N.bf16_store_bound(N.silu64(t)) if c["bf16"] else 0)
    err = (got.double() - N.silu64(t)).abs()
    worst = int((err / tol).argmax())
    miss = N.silu_miss(got, t, c["bf16"], extra)
    _report(test="conv_silu_site_range", case=site, impl=c["impl"], miss=miss, worst_t=float(t[worst]), worst_err=float(err[worst]), worst_tol=float(tol[worst]))
    assert bool(torch.isfinite(got).all())
    assert miss <= 1.0, (site, miss, float(t[worst]), float(got[worst]), float(N.silu64(t)[worst]))


# ------------------------------------------------------------------------------------------------ rms_norm
def rmsnorm(x, y, res, g, npix, C, bf16):
    L().check(L().lib().srgd_k_rmsnorm(ptr(x), ptr(y), ptr(res), ptr(g), npix, C, int(bf16), stream()), "rmsnorm")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", N.RMS_EXACT_SHAPES, ids=lambda s: s.id)
def test_rms_norm_exact_rows_incl_the_grid_stride_loops_second_trip(shape):
    s = shape
    e = N.rms_exact(s.C, s.bf16)
    launch = N.rms_launch(s.npix, s.C, s.bf16)
    dtype = torch.bfloat16 if s.bf16 else torch.float32
    r = torch.arange(s.npix, device=DEV)
    x, res, g = tiled(e.base_x, r, dtype), tiled(e.base_res, r, dtype), e.g.to(DEV)
    n = s.npix * s.C
    # out of place, with the residual
    buf, mid = guarded(n, dtype)
    rmsnorm(x, mid, res, g, s.npix, s.C, s.bf16)
    bad_res = mismatches(mid.reshape(s.npix, s.C), tiled(e.want_res, r, torch.float32))
    check_guards(buf, n, s.id)
    assert mismatches(x, tiled(e.base_x, r, torch.float32)) == 0, "input written"
    # in place, without
    buf, mid = guarded(n, dtype)
    mid.copy_(x.reshape(-1))
    rmsnorm(mid, mid, None, g, s.npix, s.C, s.bf16)
    bad = mismatches(mid.reshape(s.npix, s.C), tiled(e.want, r, torch.float32))
    check_guards(buf, n, s.id)
    _report(test="rms_norm_exact_rows", case=s.id, mismatches_residual=bad_res, mismatches_in_place=bad, elements=n, L=launch.L,
            v_trips=launch.v_trips, pixel_trips=launch.pixel_trips)
    if bad:
        k = min(s.npix, 4096)
        N.assert_exact(mid.reshape(s.npix, s.C)[-k:].float().cpu(), N.rows_of(e.want, s.npix - k, k), s.id + " (last pixels)")
    assert bad_res == 0 and bad == 0, (s.id, bad_res, bad)


@pytest.mark.parametrize("shape", N.RMS_RAGGED, ids=lambda s: s.id)
def test_rms_norm_ragged_vector_loop_against_float64(shape):
    s = shape
    v = N.rms_ragged(s)
    dtype = torch.bfloat16 if s.bf16 else torch.float32
    x, res, g = v.x.to(DEV).to(dtype), v.res.to(DEV).to(dtype), v.g.to(DEV)
    n = s.npix * s.C
    buf, mid = guarded(n, dtype)
    rmsnorm(x, mid, res, g, s.npix, s.C, s.bf16)
    got = mid.reshape(s.npix, s.C).float().cpu()
    buf2, mid2 = guarded(n, dtype)
    mid2.copy_(x.reshape(-1))
    rmsnorm(mid2, mid2, None, g, s.npix, s.C, s.bf16)
    got_plain = mid2.reshape(s.npix, s.C).float().cpu()
    _report(test="rms_norm_ragged", case=s.id, tolerance=v.tol, e32=v.e32, distance=N.distance(got, v.want),
            distance_in_place=N.distance(got_plain, v.want_plain), miss=N.within(got, v.want, v.tol, s.bf16))
    check_guards(buf, n, s.id)
    check_guards(buf2, n, s.id)
    assert N.within(got, v.want, v.tol, s.bf16) <= 1.0 and N.within(got_plain, v.want_plain, v.tol, s.bf16) <= 1.0


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [16, 64, 1024])
def test_rms_norm_edge_rows(C, bf16):
    x, g, want, rows = N.rms_edges(C, bf16)
    dtype = torch.bfloat16 if bf16 else torch.float32
    npix = x.shape[0]
    dx = x.to(DEV).to(dtype)
    buf, mid = guarded(npix * C, dtype)
    rmsnorm(dx, mid, None, g.to(DEV), npix, C, bf16)
    got = mid.reshape(npix, C).float().cpu()
    per_row = {name: N.edge_miss(got[r:r + 1], want[r:r + 1], bf16) for name, r in rows.items()}
    _report(test="rms_norm_edge_rows", case="%s_C%d" % ("bf16" if bf16 else "fp32", C), miss=per_row)
    check_guards(buf, npix * C)
    assert not got[rows["zero"]].any()
    assert bool(torch.isnan(got[rows["nan"]]).all()) and int(torch.isnan(got).any(1).sum()) == 1       # the NaN stays in its pixel
    assert N.edge_miss(got, want, bf16) <= 1.0, per_row


# ------------------------------------------------------------------------------------------------ conv1x1_split's folded RMSNorm
@pytest.mark.parametrize("f", N.FOLDED, ids=lambda f: f.id)
def test_conv1x1_split_folded_rms_norm_on_the_exact_rows(f):
    base_x, g, w, base_res, base_want, base_mag = N.folded_case(f)
    npix = f.B * f.N
    r = torch.arange(npix, device=DEV)
    x = tiled(base_x, r, torch.float32)
    res = None if base_res is None else tiled(base_res, r, torch.float32)
    buf, mid = guarded(npix * f.Cout, torch.float32)
    wh, gh = w.contiguous(), g.contiguous()
    L().check(L().lib().srgd_k_conv1x1_split_rms(ptr(x), f.Cin, f.B, f.N, ptr(wh), ptr(None), f.Cout, ptr(gh if f.kind == "pre" else None),
                                                 ptr(gh if f.kind == "post" else None), ptr(res), ptr(mid), stream()), "conv1x1_split_rms")
    torch.cuda.synchronize()
    got = mid.reshape(npix, f.Cout)
    want, mag = base_want.to(DEV)[r % N.PERIOD], base_mag.to(DEV)[r % N.PERIOD]
    exact = N.folded_exact(f)
    miss = N.folded_miss(got, want, mag, exact)
    rel = N.folded_miss(got, want, mag, False)
    _report(test="conv1x1_split_folded_rms", case=f.id, exact=exact, mismatches=miss if exact else None, miss_of_rel_fp32=rel, tiles=f.tiles)
    check_guards(buf, npix * f.Cout, f.id)
    assert miss <= (0.0 if exact else 1.0), (f.id, miss, rel)
