"""The conditioning path on the GPU against tests/cond_cases.py, through the read-only probes of include/srgd_hip_kernels.h:
``time_features`` and ``linear_rows`` of cond.hip (srgd_k_time_features, srgd_k_linear_rows), ``compute_conditioning`` of engine.hip
(srgd_k_conditioning_table on the product's engine, loaded as build_sampler loads it; srgd_k_conditioning_layout) and the row
addressing of ``gn_finalize`` (srgd_k_gn_coefficients).

  * the table layout, bit for bit, at dims 16 and 128: K + 1 rows per log-SNR value (label rows i (K + 1) + k, null row i (K + 1) + K),
    the per-block ss_offset, the scale | shift halves and ss_stride, on the designed network whose every entry names its log-SNR
    value, label, block, half and channel; K = 1 with a label, K = 1 without (both rows alike), K = 3 with labels out of order;
  * linear_rows, integer-exact: in_f in {1, 17, 63, 64, 65, 512}, out_f in {1, 3, 5, 130}, 1 and 3 rows, strides wider than the rows,
    add absent / add_stride 0 / add_stride > 0, every act, NaN in the input's padding, guard bands around y; its erf-GELU between
    the exact regions against float64; time_features at half in {1, 8, 64, 65}: exact at w = 0, sinf / cosf at arguments up to
    1700 rad against float64;
  * the table's values in float64 on synth_state_dict weights at log-SNR 0, +-1e-3, 9.2103, -10.0001, +-20 and the EDM run's
    0.25 log(sigma), with the sinusoid weights as they are and times 4 (arguments up to 1250 rad);
  * gn_finalize's row = ss_rows[b] + *step_ptr * step_mul, ss_offset, ss_stride and halves: with gamma = 0, coefB is the shift
    (beta = 0) or scale + 1 + shift (beta = 1) entry of a table whose entries encode (row, column).

  * launch_step_rows (fill_rows_kernel, fill_rows_labels_kernel) through srgd_k_step_rows on begun runs: DDPM (evals = 1) and EDM
    (evals = 2, both ev), one and two passes, with and without pass1_null, a one-label run, a no-label run and a per-image-label
    run over sub-batches with first > 0, both tile grids; every row against base = (K + 1) * ev + (label slot | K).

Measured on an MI355X (tolerances from the oracle alone, tests/test_cond_cases_cpu.py -s prints them):

    table layout   dim  16 K1_label         ss_stride  2016  mismatches 0 of 16128
    table layout   dim  16 K1_no_label      ss_stride  2016  mismatches 0 of 16128
    table layout   dim  16 K3_out_of_order  ss_stride  2016  mismatches 0 of 32256
    table layout   dim 128 K1_label         ss_stride 16128  mismatches 0 of 129024
    table layout   dim 128 K1_no_label      ss_stride 16128  mismatches 0 of 129024
    table layout   dim 128 K3_out_of_order  ss_stride 16128  mismatches 0 of 258048
    table values   dim  16 weights_as_they_are  largest |argument|  312 rad  E32 4.57e-07 tolerance 3.65e-06 GPU 2.10e-07
    table values   dim  16 sinusoid_weights_x4  largest |argument| 1250 rad  E32 3.25e-07 tolerance 2.60e-06 GPU 2.13e-07
    table values   dim 128 weights_as_they_are  largest |argument|  312 rad  E32 6.76e-07 tolerance 5.41e-06 GPU 2.61e-07
    table values   dim 128 sinusoid_weights_x4  largest |argument| 1250 rad  E32 6.26e-07 tolerance 5.01e-06 GPU 2.53e-07
    linear_rows    act 0: 144 launches, failing []
    linear_rows    act 1: 144 launches, failing []
    linear_rows    act 2: 144 launches, failing []
    linear_rows    erf-GELU sweep: tolerance 7.01e-07 GPU 1.25e-07
    time_features  half  1: w = 0 exact (GPU 0); values tolerance 4.77e-07 GPU 3.01e-08
    time_features  half  8: w = 0 exact (GPU 0); values tolerance 4.77e-07 GPU 5.91e-08
    time_features  half 64: w = 0 exact (GPU 0); values tolerance 4.77e-07 GPU 6.25e-08
    time_features  half 65: w = 0 exact (GPU 0); values tolerance 4.77e-07 GPU 5.24e-08
    gn_finalize    C  16: 12 launches (step none, 0, 1, 7; step_mul 2, 8; beta 0, 1), failing []
    gn_finalize    C  96: 12 launches (step none, 0, 1, 7; step_mul 2, 8; beta 0, 1), failing []
    gn_finalize    C 128: 12 launches (step none, 0, 1, 7; step_mul 2, 8; beta 0, 1), failing []
    step rows      ddpm one_label  21 launches, failing []
    step rows      ddpm no_label   21 launches, failing []
    step rows      ddpm per_image  21 launches, failing []
    step rows      edm  one_label  42 launches, failing []
    step rows      edm  no_label   42 launches, failing []
    step rows      edm  per_image  42 launches, failing []

Every distance is reported through test_engine_gpu._report.
"""
import ctypes as CT
import os

import pytest
import torch

from tests import cond_cases as C
from tests.test_engine_gpu import G, _report
from tests.test_kernels_gpu import DEV, L, ptr, stream

pytestmark = pytest.mark.gpu

_UNETS = {}


def unet_with(key, dim, make_sd):
    """The product's U-Net object with the state dict ``make_sd()``, built as test_engine_gpu.build_sampler builds it."""
    if key not in _UNETS:
        import logging
        from srgd_amd.config import load_config
        from srgd_amd.model import get_model
        conf = load_config(os.path.join(os.path.dirname(G), "..", "conf", "conditional_continuous_linear_df8kost_dim128.yaml"))
        conf.unet_dim = dim
        ema = get_model(conf, logging.getLogger("test"))
        ema.module.load_state_dict(make_sd(), strict=True)
        _UNETS[key] = ema.module.eval().to(torch.device("cuda")).model
    return _UNETS[key]


def engine_handle(unet):
    return unet.engine("fp32")._h


def table_layout(h):
    """({block: (ss_offset, Cout)} in the engine's order, ss_stride) as srgd_k_conditioning_layout reports them."""
    lib = L().lib()
    stride, nb = CT.c_int(), CT.c_int()
    L().check(lib.srgd_k_conditioning_layout(h, CT.byref(stride), CT.byref(nb), -1, None, 0, None, None), "conditioning_layout")
    out = {}
    for i in range(nb.value):
        name, off, cout = CT.create_string_buffer(256), CT.c_int(), CT.c_int()
        L().check(lib.srgd_k_conditioning_layout(h, None, None, i, name, 256, CT.byref(off), CT.byref(cout)), "conditioning_layout")
        out[name.value.decode()] = (off.value, cout.value)
    assert len(out) == nb.value
    return out, stride.value


def conditioning_table(h, log_snr, class_ids, stride):
    n, K = len(log_snr), len(class_ids)
    table = torch.full(((K + 1) * n, stride), float("nan"))
    ls, ids = (CT.c_float * n)(*log_snr), (CT.c_int32 * K)(*class_ids)
    L().check(L().lib().srgd_k_conditioning_table(h, ls, n, ids, K, CT.c_void_p(table.data_ptr()), stream()), "conditioning_table")
    return table


@pytest.mark.parametrize("labels", list(C.LAYOUT_LABELS), ids=str)
@pytest.mark.parametrize("dim", [16, 128])
def test_conditioning_table_layout_is_bit_exact(dim, labels):
    h = engine_handle(unet_with(("designed", dim), dim, lambda: C.designed_state_dict(dim)))
    layout, stride = table_layout(h)
    C.assert_layout_is_a_partition(layout, stride, dim)
    ids = C.LAYOUT_LABELS[labels]
    want = C.assemble(C.designed_rows(dim, C.LAYOUT_LOG_SNR, ids), layout, stride)
    got = conditioning_table(h, C.LAYOUT_LOG_SNR, ids, stride)
    bad = int((got.double() != want).sum())
    _report(test="conditioning_table_layout", dim=dim, labels=labels, mismatches=bad, entries=want.numel(), ss_stride=stride)
    C.assert_exact(got, want, "table dim %d %s" % (dim, labels))


@pytest.mark.parametrize("variant", C.VALUE_VARIANTS)
@pytest.mark.parametrize("dim", [16, 128])
def test_conditioning_table_values_against_float64(dim, variant):
    h = engine_handle(unet_with((variant, dim), dim, lambda: C.value_state_dict(dim, variant)))
    layout, stride = table_layout(h)
    C.assert_layout_is_a_partition(layout, stride, dim)
    case = C.value_case(dim, variant)
    want = C.assemble(case.want, layout, stride)
    got = conditioning_table(h, case.log_snr, case.class_ids, stride)
    d = C.distance(got, want)
    _report(test="conditioning_table_values", dim=dim, variant=variant, distance=d, tolerance=case.tol, e32=case.e32, max_arg=case.max_arg)
    assert d <= case.tol, (d, case.tol)


def test_the_probes_refuse_null_arguments():
    lib = L().lib()
    assert lib.srgd_k_time_features(None, None, 1, 1, None, stream()) == -1 and b"null" in lib.srgd_last_error()
    assert lib.srgd_k_linear_rows(None, 1, None, None, None, 1, 1, 1, 1, 0, None, 0, stream()) == -1 and b"null" in lib.srgd_last_error()
    assert lib.srgd_k_conditioning_table(None, None, 1, None, 1, None, stream()) == -1 and b"null" in lib.srgd_last_error()
    assert lib.srgd_k_conditioning_layout(None, None, None, -1, None, 0, None, None) == -1 and b"null" in lib.srgd_last_error()
    assert lib.srgd_k_gn_coefficients(None, 1, 1, 1, 4, 1, None, None, None, 0, 0, None, None, 0, None, None, stream()) == -1
    assert b"null" in lib.srgd_last_error()


# ------------------------------------------------------------------------------------------------ the raw launchers
def guarded(n):
    buf = torch.full((n + 2 * C.GUARD,), C.SENTINEL, device=DEV)
    return buf, buf[C.GUARD:C.GUARD + n]


def linear_rows(c, in_f, out_f, rows, act):
    buf, mid = guarded(rows * c.y_stride)
    dx, dW = c.x.to(DEV), c.W.to(DEV)
    db = None if c.b is None else c.b.to(DEV)
    dadd = None if c.add is None else c.add.to(DEV)
    L().check(L().lib().srgd_k_linear_rows(ptr(dx), c.x_stride, ptr(dW), ptr(db), ptr(mid), c.y_stride, rows, in_f, out_f, act, ptr(dadd),
                                           c.add_stride, stream()), "linear_rows")
    out = buf.cpu()
    y = out[C.GUARD:C.GUARD + rows * c.y_stride].reshape(rows, c.y_stride)
    untouched = bool((out[:C.GUARD] == C.SENTINEL).all()) and bool((out[-C.GUARD:] == C.SENTINEL).all()) and bool((y[:, out_f:] == C.SENTINEL).all())
    return y[:, :out_f], untouched


@pytest.mark.parametrize("act", [C.ACT_NONE, C.ACT_GELU, C.ACT_SILU_IN], ids=["none", "gelu", "silu_in"])
def test_linear_rows_is_integer_exact_at_every_edge(act):
    bad = []
    n = 0
    for in_f in C.LIN_IN:
        for out_f in C.LIN_OUT:
            for rows in C.LIN_ROWS:
                for add in C.LIN_ADD:
                    c = C.lin_case(in_f, out_f, rows, add, act)
                    y, untouched = linear_rows(c, in_f, out_f, rows, act)
                    n += 1
                    if not untouched or bool((y != c.want).any()):
                        bad.append((in_f, out_f, rows, add, untouched, int((y != c.want).sum())))
    _report(test="linear_rows_exact", act=act, launches=n, failing=bad)
    assert not bad, bad


def test_linear_rows_erf_gelu_between_its_exact_regions():
    s, want, tol = C.gelu_sweep()
    buf, mid = guarded(s.numel())
    dx, dW = torch.ones(1, device=DEV), s.to(DEV).reshape(-1, 1).contiguous()
    L().check(L().lib().srgd_k_linear_rows(ptr(dx), 1, ptr(dW), ptr(None), ptr(mid), s.numel(), 1, 1, s.numel(), C.ACT_GELU, ptr(None), 0,
                                           stream()), "linear_rows")
    d = C.distance(mid.cpu(), want)
    _report(test="linear_rows_gelu_sweep", distance=d, tolerance=tol)
    assert d <= tol, (d, tol)


@pytest.mark.parametrize("half", C.TF_HALF)
def test_time_features_layout_and_values(half):
    lib = L().lib()
    for rows in C.TF_ROWS:
        for kind in ("zero", "values"):
            x, w, want, tol = C.tf_case(half, rows, kind)
            nf = 2 * half + 1
            buf, mid = guarded(rows * nf)
            dx, dw = x.to(DEV), w.to(DEV)
            L().check(lib.srgd_k_time_features(ptr(dx), ptr(dw), half, rows, ptr(mid), stream()), "time_features")
            out = buf.cpu()
            got = out[C.GUARD:C.GUARD + rows * nf].reshape(rows, nf)
            d = C.distance(got, want)
            _report(test="time_features", half=half, rows=rows, kind=kind, distance=d, tolerance=tol)
            assert bool((out[:C.GUARD] == C.SENTINEL).all()) and bool((out[-C.GUARD:] == C.SENTINEL).all()), "guard band written"
            assert d <= tol, (half, rows, kind, d, tol)


# ------------------------------------------------------------------------------------------------ gn_finalize's row addressing
@pytest.mark.parametrize("C_groups", C.GNC_C, ids=lambda v: "C%d" % v[0])
def test_gn_finalize_reads_its_own_row_offset_and_halves(C_groups):
    Cc, groups = C_groups
    lib = L().lib()
    B, hw, nslots = len(C.GNC_ROWS), 64, 2
    table, stride = C.gnc_table(Cc)
    dt = table.to(DEV)
    rows = torch.tensor(C.GNC_ROWS, dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(Cc)
    partial = torch.rand(B, groups, nslots, 2, generator=g).to(DEV) + 1.0           # any finite statistics: gamma = 0 removes them
    gamma = torch.zeros(Cc, device=DEV)
    bad = []
    for step, mul in C.GNC_STEPS:
        dstep = None if step is None else torch.tensor([step], dtype=torch.int32, device=DEV)
        for beta1 in (False, True):
            beta = torch.full((Cc,), 1.0 if beta1 else 0.0, device=DEV)
            bufA, cA = guarded(B * Cc)
            bufB, cB = guarded(B * Cc)
            L().check(lib.srgd_k_gn_coefficients(ptr(partial), nslots, B, hw, Cc, groups, ptr(gamma), ptr(beta), ptr(dt), stride, C.GNC_OFFSET,
                                                 ptr(rows), ptr(dstep), mul, ptr(cA), ptr(cB), stream()), "gn_coefficients")
            a, b = bufA.cpu(), bufB.cpu()
            want = C.gnc_want(Cc, beta1, step, mul)
            ok = bool((a[C.GUARD:-C.GUARD] == 0).all()) and torch.equal(b[C.GUARD:-C.GUARD].reshape(B, Cc), want)
            for band in (a[:C.GUARD], a[-C.GUARD:], b[:C.GUARD], b[-C.GUARD:]):
                ok = ok and bool((band == C.SENTINEL).all())
            if not ok:
                bad.append((step, mul, beta1))
    _report(test="gn_coefficients_rows", C=Cc, launches=2 * len(C.GNC_STEPS), failing=bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ launch_step_rows
def begin_run(eng, kind, class_id):
    """A begun run of STEP_IMAGES equal images on the engine: two even-grid and one odd-grid tile each, three steps."""
    from srgd_amd._lib import EdmScalars, SamplerGeometry, StepScalars
    T, n = C.STEP_TILE, 3
    geo = SamplerGeometry(H=2 * T, W=T, Hp=2 * T, Wp=T, left=0, top=0, inner_l=0, inner_t=0, inner_r=T, inner_b=2 * T, tile=T,
                          n_even=len(C.STEP_TILES[0]), n_odd=len(C.STEP_TILES[1]), n_images=C.STEP_IMAGES)
    cond01 = torch.rand(C.STEP_IMAGES, 3, 2 * T, T, device=DEV)
    canvas = torch.empty_like(cond01)
    if kind == "ddpm":
        eng.sampler_begin(geo, cond01, canvas, C.STEP_TILES[0], C.STEP_TILES[1], [StepScalars() for _ in range(n)],
                          [1.0 - 0.5 * i for i in range(n)], class_id)
    else:
        eng.edm_begin(geo, cond01, canvas, C.STEP_TILES[0], C.STEP_TILES[1], [EdmScalars() for _ in range(n)],
                      [0.5 - 0.25 * i for i in range(2 * n)], class_id)
    torch.cuda.synchronize()
    return cond01, canvas


@pytest.mark.parametrize("mode", list(C.STEP_LABEL_MODES))
@pytest.mark.parametrize("kind", ["ddpm", "edm"])
def test_launch_step_rows_selects_the_rows_of_the_formula(kind, mode):
    eng = unet_with(("step_rows", 16), 16, lambda: C.value_state_dict(16, "weights_as_they_are")).engine("fp32")
    spec = C.STEP_LABEL_MODES[mode]
    keep = begin_run(eng, kind, spec[0] if mode == "per_image" else spec)
    if mode == "per_image":
        eng.sampler_image_labels(spec)
    lib = L().lib()
    bad = []
    launches = C.step_launches(mode, 1 if kind == "ddpm" else 2)
    for parity, nb, nt, first, ev, null in launches:
        rows = (CT.c_int32 * nb)(*([-1] * nb))
        L().check(lib.srgd_k_step_rows(eng._h, parity, nb, nt, first, ev, null, rows, stream()), "step_rows")
        want = C.step_rows_want(mode, parity, nb, nt, first, ev, null).tolist()
        if list(rows) != want:
            bad.append(((parity, nb, nt, first, ev, null), list(rows), want))
    _report(test="launch_step_rows", kind=kind, mode=mode, launches=len(launches), failing=bad)
    del keep
    assert not bad, bad[:4]
    # a batch outside the parity's grid is refused, not launched
    assert lib.srgd_k_step_rows(eng._h, 1, 4, 4, 0, 0, 0, (CT.c_int32 * 4)(), stream()) == -1
    assert lib.srgd_k_step_rows(None, 0, 1, 1, 0, 0, 0, None, stream()) == -1 and b"null" in lib.srgd_last_error()

