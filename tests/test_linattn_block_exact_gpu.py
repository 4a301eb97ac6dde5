"""The fused bf16 LinearAttention block (linattn_fused.hip at C = 128, linattn_fused256.hip at C = 256: la1 -> la_combine -> la2)
against float64, on the closed-form cases of tests/linattn_block_cases.py, at the smallest shapes that reach every launch-shape
branch: one tile, one strip with and without a ring wrap, a ragged last strip at each strip length, and the persistent la2 loop at
each depth with a short last workgroup.

Per case: y, the normalised context and the row norms (read through srgd_k_linattn_block_fused_probe) within the gates of the
cases module - which come from the CPU emulation's error against float64, never from the kernels; entries of a batch bit-identical
to their solo calls; a guard band around y untouched; at two shapes the MX-fp8 twin of y bit-identical to srgd_k_quant_mxfp8(y).
The strip length and tiles-per-workgroup of every launch are read back through the same entry point, never computed here, and
test_shapes_cover_every_launch_branch holds the shape list to every value of both.  Batches are one image rolled by per-entry
offsets (the block is equivariant under permutations of the positions), so one float64 reference serves the whole batch.
Every measured error goes to the parity report of tests/test_kernels_gpu.py (`_report_k`) beside its gate."""
import ctypes as C

import pytest
import torch

from tests import linattn_block_cases as LC
from tests.test_kernels_gpu import _report_k as _report

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096                                            # bf16 elements on either side of y

SINGLE_STRIP = [(1, 64), (1, 128), (1, 192), (1, 256)]
RAGGED_STRIP = [(2, 320), (1, 2112), (1, 16576), (1, 65600)]                        # strips of 256, 512, 1024, 2048
# persistent la2: the smallest (B, N) per loop depth whose tile count is no multiple of the depth (C = 128: 2, 4, 8, 16; C = 256:
# 4, 8, 16, 32), the depth-2 launch of C = 256 (its tile counts are always even: no short workgroup exists), and the two ends of
# the launcher's range, B = 64 x N = 2112 and B = 1024 x N = 1088 (0.6 GB of x at C = 256)
PERSISTENT = [(512, 128), (512, 192), (512, 320), (512, 576), (512, 1088), (64, 2112), (1024, 1088)]
STRIPS = {256, 512, 1024, 2048}
DEPTHS = {128: {1, 2, 4, 8, 16}, 256: {1, 2, 4, 8, 16, 32}}
TWIN_SHAPES = [(1, 2112), (512, 320)]                   # one ragged strip, one persistent loop


def _id(s):
    return "B%d_N%d" % s


def L():
    from srgd_amd import _lib
    return _lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def offsets(B, N):
    """Roll of each batch entry: none a multiple of 64 except the unrolled first and (B > 2) last entry."""
    r = [((b * 37) % (N // 64)) * 64 + 1 + b % 63 for b in range(B)]
    r[0] = 0
    if B > 2:
        r[-1] = 0
    return torch.tensor(r)


def host_weights(P):
    return [P["wqkv"].float().contiguous(), P["g1"].float().contiguous(), P["wout"].float().contiguous(),
            P["bout"].float().contiguous(), P["g2"].float().contiguous()]


def run_block(x_dev, P, twin=False):
    """x_dev [B, N, C] bf16 on the GPU -> y (inside its guard band), ctxn, rinv, twin, (strip, tiles_per_wg) as the launch reports."""
    B, N, Cc = x_dev.shape
    buf = torch.full((B * N * Cc + 2 * GUARD,), -7.0, device=DEV, dtype=torch.bfloat16)
    y = buf[GUARD:GUARD + B * N * Cc].view(B, N, Cc)
    ctxn = torch.full((B * 4, 32, 32), float("nan"), device=DEV)
    rinv = torch.full((B, N), float("nan"), device=DEV)
    yq = torch.zeros(B * N * Cc, device=DEV, dtype=torch.uint8) if twin else None
    ys = torch.zeros(B * N * Cc // 32, device=DEV, dtype=torch.uint8) if twin else None
    strip, tpw = C.c_int(-1), C.c_int(-1)
    hw = host_weights(P)
    L().check(L().lib().srgd_k_linattn_block_fused_probe(ptr(x_dev), ptr(y), B, N, Cc, *[ptr(t) for t in hw], ptr(ctxn), ptr(rinv),
                                                         ptr(yq), ptr(ys), C.byref(strip), C.byref(tpw), stream()), "probe")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == -7.0).all()) and bool((buf[GUARD + B * N * Cc:] == -7.0).all()), "guard band around y overwritten"
    return {"y": y, "ctxn": ctxn.view(B, 4, 32, 32), "rinv": rinv, "yq": yq, "ys": ys, "strip": strip.value, "tpw": tpw.value}


def batch_of(case, B):
    """The case's image rolled per entry, on the GPU: x [B, N, C] bf16 and the gather index [B, N] (entry b, row n <- image row)."""
    N = case["N"]
    x = case["x"].to(torch.bfloat16).to(DEV)
    idx = (torch.arange(N)[None, :] - offsets(B, N)[:, None]) % N
    idx = idx.to(DEV)
    return x[idx].contiguous(), idx


_WANT = {}


def want_of(case):
    key = (case["family"], case["C"], case["N"])
    if key not in _WANT:
        _WANT.clear()                                      # one float64 reference alive at a time, shared by the tests of a case
        _WANT[key] = {k: v.to(DEV) for k, v in LC.expected(case).items()}
    return _WANT[key]


def check_case(family, Cc, B, N, twin=False):
    case = LC.make_case(family, Cc, N)
    assert float((case["x"] - LC.bf(case["x"])).abs().max()) == 0.0
    want = want_of(case)
    x_dev, idx = batch_of(case, B)
    got = run_block(x_dev, case["P"], twin)
    assert got["strip"] == LC.design_strip(N), "the cases were laid out for another strip length"
    worst = {t: (0.0, 0.0) for t in LC.TENSORS}
    step = max(1, (1 << 24) // (N * Cc))                   # entries per comparison chunk
    for b0 in range(0, B, step):
        sl = slice(b0, min(B, b0 + step))
        for t, g, w in (("y", got["y"][sl], want["y"][idx[sl]]), ("rinv", got["rinv"][sl], want["rinv"][idx[sl]]),
                        ("ctxn", got["ctxn"][sl], want["ctxn"][None].expand(sl.stop - sl.start, -1, -1, -1))):
            ex, err = LC.excess(g, w, family, Cc, t)
            worst[t] = (max(worst[t][0], ex), max(worst[t][1], err))
    for t in LC.TENSORS:
        a, b = LC.GATES[(family, Cc, t)]
        print(f"linattn block {family} C={Cc} B={B} N={N} {t}: max|err| {worst[t][1]:.4g}, worst element {worst[t][0]:.3f} of its gate "
              f"(a={a}, b={b}); strip {got['strip']}, tiles/wg {got['tpw']}")
        _report(kind="linattn_block_exact", family=family, C=Cc, B=B, N=N, tensor=t, max_abs_err=worst[t][1],
                worst_over_gate=worst[t][0], gate_a=a, gate_b=b, strip=got["strip"], tiles_per_wg=got["tpw"])
    # every entry bit-identical to its solo call: the unrolled image (first and last entry) and the first rolled one
    if B > 1:
        solo = run_block(x_dev[:1].contiguous(), case["P"])
        for b in ([0, B - 1] if B > 2 else [0]):
            for t in LC.TENSORS:
                assert torch.equal(got[t][b], solo[t][0]), (t, b)
        solo1 = run_block(x_dev[1:2].contiguous(), case["P"])
        for t in LC.TENSORS:
            assert torch.equal(got[t][1], solo1[t][0]), (t, 1)
    if twin:
        q = torch.zeros_like(got["yq"])
        s = torch.zeros_like(got["ys"])
        yc = got["y"].contiguous()
        L().check(L().lib().srgd_k_quant_mxfp8(ptr(yc), ptr(q), ptr(s), B * N, Cc, stream()), "quant")
        torch.cuda.synchronize()
        assert torch.equal(got["yq"], q) and torch.equal(got["ys"], s), "MX-fp8 twin differs from quant_mxfp8(y)"
    for t in LC.TENSORS:
        assert worst[t][0] <= 1.0, (t, worst[t])
    return got


@pytest.mark.parametrize("Cc", [128, 256])
@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("shape", SINGLE_STRIP, ids=_id)
def test_single_strip(shape, family, Cc):
    check_case(family, Cc, *shape)


@pytest.mark.parametrize("Cc", [128, 256])
@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("shape", RAGGED_STRIP, ids=_id)
def test_ragged_last_strip(shape, family, Cc):
    B, N = shape
    assert N % LC.design_strip(N) != 0
    check_case(family, Cc, B, N)


@pytest.mark.parametrize("Cc", [128, 256])
@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("shape", PERSISTENT, ids=_id)
def test_persistent_la2(shape, family, Cc):
    check_case(family, Cc, *shape)


@pytest.mark.parametrize("Cc", [128, 256])
@pytest.mark.parametrize("shape", TWIN_SHAPES, ids=_id)
def test_mxfp8_twin_is_quant_of_y(shape, Cc):
    check_case("gaussian", Cc, *shape, twin=True)


def test_shapes_cover_every_launch_branch():
    """Every strip length and every tiles-per-workgroup value, as the launches themselves report them; and among the persistent
    launches one with a short last workgroup per depth (where a short one exists)."""
    seen = {128: {"strip": set(), "tpw": set(), "short": set()}, 256: {"strip": set(), "tpw": set(), "short": set()}}
    for Cc in (128, 256):
        P = LC.make_case("gaussian", Cc, 64)["P"]
        for B, N in SINGLE_STRIP + RAGGED_STRIP + PERSISTENT:
            got = run_block(torch.ones(B, N, Cc, device=DEV, dtype=torch.bfloat16), P)
            seen[Cc]["strip"].add(got["strip"])
            seen[Cc]["tpw"].add(got["tpw"])
            ntiles = N // LC.tile_px(Cc)
            if ntiles > got["tpw"] and ntiles % got["tpw"]:
                seen[Cc]["short"].add(got["tpw"])
            if (B, N) in RAGGED_STRIP:
                assert N % got["strip"] and N > got["strip"], (B, N, got["strip"])
            if (B, N) in SINGLE_STRIP:
                assert N <= got["strip"]
        print(f"linattn block C={Cc}: strips {sorted(seen[Cc]['strip'])}, tiles/wg {sorted(seen[Cc]['tpw'])}, "
              f"with a short last workgroup {sorted(seen[Cc]['short'])}")
        _report(kind="linattn_block_coverage", C=Cc, strips=sorted(seen[Cc]["strip"]), tiles_per_wg=sorted(seen[Cc]["tpw"]),
                short_last_wg=sorted(seen[Cc]["short"]))
        assert seen[Cc]["strip"] == STRIPS
        assert seen[Cc]["tpw"] == DEPTHS[Cc]
        assert seen[Cc]["short"] >= DEPTHS[Cc] - {1} - ({2} if Cc == 256 else set())
