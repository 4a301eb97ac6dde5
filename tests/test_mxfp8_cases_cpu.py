"""tests/mxfp8_cases.py proved on the CPU: the conditions its docstrings state, the coverage the sweep and the launch shapes
claim, the undecided-share caps of the gaussian family, and - the point of the file - that the assertions the GPU tests use
reject every wrong quantiser of `VALUE_MUTANTS`, `LAYOUT_MUTANTS` and the section-specific mutants on the cases' own data."""
import pytest
import torch
import torch.nn.functional as F

from oracle import mxfp8 as MX
from tests import mxfp8_cases as M


def rejected(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------ the reference quantiser
def test_reference_quantiser_equals_the_oracle_on_every_section_1_tensor():
    for x, q, s in (M.sweep(), M.nonfinite(), M.launch_case(1000, 96)[:3], M.launch_case(4096 * 1024, 32)[:3]):
        rq, rs = M.ref_quantize(x.float())
        M.assert_bytes(rq, rs, q, s)
    w = M.weight_case(9, 128, 128, 61, with_subnormal=True)[0]
    rq, rs = M.ref_quantize(w)
    wq, ws, _ = MX.quantize(w)
    M.assert_bytes(rq, rs, wq, ws)


# ------------------------------------------------------------------------------------------------ 1. sweep coverage
def test_sweep_reaches_every_code_both_scale_clamps_and_thousands_of_ties():
    x, q, s = M.sweep()
    assert x.shape[1] == 32 and torch.isfinite(x.float()).all()
    codes = set(q.unique().tolist())
    assert codes == set(range(256)) - {0x7F, 0xFF}                       # all 254 non-NaN e4m3 codes
    bits = x.view(torch.int16).to(torch.int32) & 0xFFFF
    amax_exp = ((bits >> 7) & 0xFF).amax(1)
    assert set(amax_exp.unique().tolist()) == set(range(255))            # every biased exponent a bf16 maximum can carry
    clamped = (amax_exp >= 1) & (amax_exp <= 7)                           # exponent - 8 (+ 1) is negative there
    assert bool(clamped.any()) and bool((s[clamped] == 0).all())          # scale byte 0 reached by clamping
    assert int(s.max()) >= 246 and {246, 247} <= set(s.unique().tolist())
    amax_bits = (bits & 0x7FFF).amax(1)
    for m in M.SWEEP_MANTISSAS:
        for sign in (0, 0x8000):
            hit = ((bits & 0x7FFF) == amax_bits[:, None]) & ((bits & 0x8000) == sign) & ((bits & 0x7F) == m)
            assert int(hit.any(1).sum()) >= 255 * M.SWEEP_BLOCKS_PER_MAX // 2, (m, sign)
    # bf16 subnormal elements and both zeros occur
    assert bool(((bits & 0x7F80) == 0).logical_and((bits & 0x7F) != 0).any()) and bool((bits == 0x8000).any()) and bool((bits == 0).any())
    down, up = M.tie_counts(x.float(), q, s)
    assert down >= 1000 and up >= 1000, (down, up)
    # the maximum sits in every lane position
    pos = (bits & 0x7FFF).argmax(1)
    assert set(pos.unique().tolist()) == set(range(32))


def test_nonfinite_blocks_follow_the_rule_of_srgd_hip_h():
    x, q, s = M.nonfinite()
    xf = x.float()
    inf_blocks = torch.isinf(xf).any(1)
    assert bool(inf_blocks.any()) and bool((s[inf_blocks, 0] == 247).all())          # biased exponent 255 - 8
    assert bool((q[xf == float("inf")] == 0x7E).all()) and bool((q[xf == float("-inf")] == 0xFE).all())
    assert bool(((q[torch.isnan(xf)] & 0x7F) == 0x7F).all())
    # a NaN takes no part in the maximum: the block's scale and every other byte are those of the block with the NaN zeroed
    nan_only = torch.isnan(xf).any(1) & ~inf_blocks
    assert bool(nan_only.any())
    cq, cs, _ = MX.quantize(torch.where(torch.isnan(xf), torch.zeros_like(xf), xf))
    assert torch.equal(cs[nan_only], s[nan_only]) and torch.equal(cq[~torch.isnan(xf)], q[~torch.isnan(xf)])
    # finite elements beside an infinity are scaled by 2^-120: the largest finite bf16 lands on a non-zero code
    assert int(q[63, 0]) not in (0x00, 0x80)


def test_launch_shapes_cover_every_branch():
    L = [M.quant_launch(*sh) for sh in M.LAUNCH_SHAPES]
    assert {l.B for l in L} >= {1, 2, 4096}
    assert {l.vpp for l in L} >= {4, 12, 16, 48, 128, 192}
    trips = set().union(*(l.trips for l in L))
    assert {(1, 0), (1, 1), (1, 2), (1, 3), (0, 1)} <= trips, trips       # a four-vector trip followed by 0, 1, 2, 3 single trips
    for sh, l in zip(M.LAUNCH_SHAPES, L):
        assert l.n % 4 == 0 and l.stride % 4 == 0 and l.n * l.B == sh[0] * sh[1] // 8 and l.n < 2 ** 31
    for (npix, C) in M.LAUNCH_SHAPES:
        x, q, s, P = M.launch_case(npix, C)
        assert x.shape == (P, C) and (P == npix or (P == M.LAUNCH_PERIOD and npix % P != 0))
        assert int(s.min()) == 0 and len(s.unique()) > 20
    G = {sh: M.gn_launch(*sh) for sh in M.GN_SHAPES}
    assert {(l.hoist, l.vpp) for l in G.values()} == {(True, 16), (True, 128), (False, 12), (False, 48)}


@pytest.mark.parametrize("name", sorted(M.VALUE_MUTANTS))
def test_section_1_rejects_value_mutant(name):
    x, q, s = M.sweep()
    mq, ms = M.ref_quantize(x.float(), **M.VALUE_MUTANTS[name])
    if name == "amax_over_the_wrong_32":                     # needs more than one block per pixel
        x, q, s, _ = M.launch_case(1000, 96)
        mq, ms = M.ref_quantize(x.float(), **M.VALUE_MUTANTS[name])
    assert rejected(M.assert_bytes, mq, ms, q, s)


@pytest.mark.parametrize("name", sorted(M.LAYOUT_MUTANTS))
def test_section_1_rejects_layout_mutant(name):
    for npix, C in ((1000, 96), (64, 1024)):
        x, q, s, _ = M.launch_case(npix, C)
        assert rejected(M.assert_bytes, *M.LAYOUT_MUTANTS[name](q, s), q, s)


def test_guard_assertion_rejects_a_stray_byte():
    buf = torch.full((M.S_GUARD * 2 + 40,), M.SENTINEL, dtype=torch.uint8)
    M.assert_guards(buf, 40, M.S_GUARD)
    for i in (M.S_GUARD - 1, M.S_GUARD + 40):
        b = buf.clone()
        b[i] = 0
        assert rejected(M.assert_guards, b, 40, M.S_GUARD)


# ------------------------------------------------------------------------------------------------ 2. gn_apply_silu_mxfp8
@pytest.mark.parametrize("shape", M.GN_SHAPES, ids=lambda s: "B%d_hw%d_C%d" % s)
def test_gn_exact_family_is_exact_and_robust(shape):
    B, hw, C = shape
    c = M.gn_exact(B, hw, C)
    x, a, b = c.x.float(), c.a, c.b
    assert torch.equal(c.x.double(), (c.t - b.double()[:, None, :]) / a.double()[:, None, :])         # integers, exact in bf16
    assert float(x.abs().max()) <= 256 and torch.equal(x, x.round())
    t32 = a[:, None, :] * x + b[:, None, :]                                  # exact in fp32 whether or not it is contracted
    assert torch.equal(t32.double(), c.t) and torch.equal(torch.addcmul(b[:, None, :].expand_as(x), a[:, None, :].expand_as(x), x).double(), c.t)
    pos = c.t >= M.SILU_ID_MIN
    assert bool((pos | (c.t <= M.SILU_ZERO_MAX)).all()) and 0.05 < float((~pos).double().mean()) < 0.25
    assert torch.equal(F.silu(t32[pos]), t32[pos])                           # fp32 SiLU is the identity there ...
    assert bool((torch.exp(-t32[~pos]) == float("inf")).all())               # ... and x * (1 / inf) = -0 here
    # coefficients: powers of two and small integers, distinct within a vector, between the lanes of a block, between samples
    assert torch.equal(torch.frexp(a)[0], torch.full_like(a, 0.5)) and torch.equal(b, b.round()) and float(b.abs().max()) <= 128
    pair = a.long() * 1000 + b.long()
    v = pair.reshape(B, C // 8, 8)
    assert all(len(set(v[i, j].tolist())) == 8 for i in range(B) for j in range(0, C // 8, 5))
    blk = pair.reshape(B, C // 32, 4, 8)
    assert bool((blk[:, :, 0] != blk[:, :, 1]).all()) and bool((blk[:, :, 1] != blk[:, :, 2]).all()) and bool((blk[:, :, 2] != blk[:, :, 3]).all())
    assert bool((pair[0] != pair[1]).all())
    # every block maximum has mantissa 1.5, every scaled element is a code point; both neighbouring blocks and pixels differ
    amax = c.y.float().abs().reshape(B, hw, C // 32, 32).amax(-1)
    assert bool(((amax.view(torch.int32) & 0x7FFFFF) == 0x400000).all())
    _, _, deq = MX.quantize(c.y.float())
    assert torch.equal(deq, c.y.float()) and bool((c.q[~pos] == 0x80).all())
    assert bool((c.s[:, :, 1:] != c.s[:, :, :-1]).all()) and bool((c.s[:, 1:] != c.s[:, :-1]).all())
    # a 1-ulp error of the reciprocal (y = t * (1 +- 2^-23)) moves no byte
    for f in (1 - 2.0 ** -23, 1 + 2.0 ** -23):
        q2, s2, _ = MX.quantize((c.y * f).float())
        M.assert_bytes(q2, s2, c.q, c.s)


@pytest.mark.parametrize("shape", M.GN_SHAPES, ids=lambda s: "B%d_hw%d_C%d" % s)
def test_gn_families_reject_the_coefficient_and_precision_mutants(shape):
    B, hw, C = shape
    e = M.gn_exact(B, hw, C)
    for kw in (dict(coef_vector_shift=1), dict(coef_vector_shift=-1), dict(sample0_coefs=True)):
        mq, ms, _, _ = M.gn_reference(e.x, e.a, e.b, **kw)
        assert rejected(M.assert_bytes, mq, ms, e.q, e.s), kw
    g = M.gn_gaussian(B, hw, C)
    M.assert_gn_gaussian(g.q, g.s, g)
    for kw in (dict(coef_vector_shift=1), dict(sample0_coefs=True), dict(round_y_to_bf16=True)):
        mq, ms, _, _ = M.gn_reference(g.x, g.a, g.b, **kw)
        assert rejected(M.assert_gn_gaussian, mq, ms, g), kw
    for name, kw in M.VALUE_MUTANTS.items():
        if name in ("step_up_at_ge_1.75", "round_half_away"):       # need a maximum of exactly 1.75 * 2^k / exact ties: fp32 Gaussian
            continue                                              # values have neither, section 1's sweep has both by design
        mq, ms = M.ref_quantize(g.y.float(), **kw)
        assert rejected(M.assert_gn_gaussian, mq, ms, g), name
    for name, fn in M.LAYOUT_MUTANTS.items():
        assert rejected(M.assert_gn_gaussian, *fn(g.q, g.s), g), name
        assert rejected(M.assert_bytes, *fn(e.q, e.s), e.q, e.s), name


@pytest.mark.parametrize("shape", M.GN_SHAPES, ids=lambda s: "B%d_hw%d_C%d" % s)
def test_gn_gaussian_undecided_shares_stay_under_the_cap(shape):
    g = M.gn_gaussian(*shape)
    blocks, elems = M.undecided_shares(g)
    print("undecided share: blocks %.3g elements %.3g" % (blocks, elems))
    assert blocks <= M.UNDECIDED_CAP and elems <= M.UNDECIDED_CAP, (blocks, elems)
    # an fp32 evaluation with correctly rounded exp and division lies inside the decided set's promise
    t32 = g.a[:, None, :] * g.x.float() + g.b[:, None, :]
    q32, s32, _ = MX.quantize(t32 / (1 + torch.exp(-t32)))
    M.assert_gn_gaussian(q32, s32, g)


# ------------------------------------------------------------------------------------------------ 3. the fused twins
def _twin_cases():
    for v in M.TWIN_VARIANTS_BF16:
        yield "bf16_" + v, lambda v=v: M.twin_conv_case(3, v)
    for v in M.TWIN_VARIANTS_MX:
        yield "mx_" + v, lambda v=v: M.twin_conv_case(4, v)
    for t in M.TWIN_3X3:
        yield "3x3_" + t[0], lambda t=t: M.twin_conv3x3_case(t[0])


@pytest.mark.parametrize("name,make", list(_twin_cases()), ids=[n for n, _ in _twin_cases()])
def test_twin_cases_have_diverse_scales_and_reject_the_mutants(name, make):
    c = make()
    stored = M.stored_nhwc(c.want)
    assert tuple(stored.shape) == tuple(c.out_shape)
    q, s, _ = MX.quantize(stored.float())
    M.assert_scale_diversity(s, name)
    M.assert_twin(q, s, stored)
    for mname, kw in M.VALUE_MUTANTS.items():
        if mname in ("step_up_at_ge_1.75", "flush_e4m3_subnormals"):       # need designed values: sections 1 and 4 have them
            continue
        mq, ms = M.ref_quantize(stored.float(), **kw)
        assert rejected(M.assert_twin, mq, ms, stored), mname
    for mname, fn in M.LAYOUT_MUTANTS.items():
        assert rejected(M.assert_twin, *fn(q, s), stored), mname
    if name.endswith("pixel_shuffle"):
        pre = F.pixel_unshuffle(c.want, 2)                   # the tensor before the shuffle: [B, Cout, H, W]
        mq, ms = M.unshuffled_twin(pre)
        assert mq.numel() == q.numel() and rejected(M.assert_twin, mq, ms, stored)


@pytest.mark.parametrize("cfg", [(B, hw, C, r) for (B, hw, C) in M.TWIN_GN for r in (True, False)], ids=lambda c: "B%d_hw%d_C%d_res%d" % c)
def test_twin_gn_cases_have_diverse_scales_and_reject_the_mutants(cfg):
    B, hw, C, r = cfg
    c = M.twin_gn_case(B, hw, C, r)
    stored = c.want.to(torch.bfloat16)
    q, s, _ = MX.quantize(stored.float())
    M.assert_scale_diversity(s.reshape(B, 1, hw, C // 32))
    for mname, fn in M.LAYOUT_MUTANTS.items():
        assert rejected(M.assert_twin, *fn(q, s), stored), mname
    for mname in ("amax_over_16_channels", "amax_over_the_wrong_32", "ocp_rule"):
        assert rejected(M.assert_twin, *M.ref_quantize(stored.float(), **M.VALUE_MUTANTS[mname]), stored), mname
    # the one-slot partial sums are the statistics of x
    xg = c.x.double().reshape(B, hw, c.groups, C // c.groups)
    assert torch.allclose(c.partial[:, :, 0, 0].double(), xg.sum((1, 3)), rtol=1e-6)


# ------------------------------------------------------------------------------------------------ 4. host weight quantisers
def test_weight_blocks_hold_the_designed_edges_and_reject_the_mutants():
    w, bias, deq = M.weight_case(9, 128, 128, 61, with_subnormal=True)
    blk = w.reshape(-1, 32)
    q, s, _ = MX.quantize(blk)
    amax = blk.abs().amax(1)
    mant = amax.view(torch.int32) & 0x7FFFFF
    normal = (amax.view(torch.int32) >> 23) > 0
    assert int((normal & (mant == 0x600000)).sum()) > 100 and int((normal & (mant == 0x600001)).sum()) > 100       # 1.75 and one float above
    assert int((normal & (mant == 0)).sum()) > 100                                        # exact powers of two
    assert int((amax == 0).sum()) > 100 and int(((amax > 0) & ~normal).sum()) == 1          # all-zero blocks, one fp32-subnormal block
    assert len(s.unique()) > 50
    down, up = M.tie_counts(blk, q, s)
    assert down > 1000 and up > 1000
    codes = q & 0x7F
    assert int(((codes > 0) & (codes < 8)).sum()) > 1000                                   # e4m3 subnormals of their block
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)                               # every dequantised weight is exact in bf16
    M.assert_weights_read_back(deq.clone(), deq, bias)
    # a wrong host quantiser, read back exactly, is rejected
    for name, kw in list(M.VALUE_MUTANTS.items()) + [("pow2_off", dict(log2="pow2_off"))]:
        if name in ("amax_over_the_wrong_32",):
            continue
        mq, ms = M.ref_quantize(blk, **kw)
        mdeq = (M.decode_e4m3(mq).double() * torch.ldexp(torch.ones(ms.shape, dtype=torch.float64), ms.to(torch.int64) - 127)).float()
        assert rejected(M.assert_weights_read_back, mdeq.reshape(deq.shape), deq, bias), name
    wi, bi, deqi = M.weight_case(1, 256, 128, 62, int_bias=True)
    got = (deqi.double() + bi.double()[:, None, None]).float().to(torch.bfloat16).float()
    M.assert_weights_read_back(got, deqi, bi)
    mq, ms = M.ref_quantize(wi.reshape(-1, 32), log2="pow2_off")
    mdeq = (M.decode_e4m3(mq).double() * torch.ldexp(torch.ones(ms.shape, dtype=torch.float64), ms.to(torch.int64) - 127)).float().reshape(deqi.shape)
    assert rejected(M.assert_weights_read_back, (mdeq + bi[:, None, None]).to(torch.bfloat16).float(), deqi, bi)


def test_one_hot_convolution_reads_every_weight_back_on_the_cpu():
    w, bias, deq = M.weight_case(9, 128, 128, 61)
    x, sites = M.onehot_3x3(128, 8, 32)
    xq = M._mx_deq(x)
    assert torch.equal(xq, x)                                # the one-hot activation quantises exactly
    q, s, _ = MX.quantize(x.permute(0, 2, 3, 1).contiguous())
    assert set(q.unique().tolist()) == {0, 0x78} and set(s.unique().tolist()) == {0, 119}       # element 256, scale byte 119
    w_oihw = w.permute(0, 2, 1).reshape(128, 128, 3, 3)
    assert torch.equal(MX.quantize_conv_weight(w_oihw), deq.permute(0, 2, 1).reshape(128, 128, 3, 3))
    out = F.conv2d(x.double(), MX.quantize_conv_weight(w_oihw).double(), bias.double(), padding=1).float()
    M.assert_weights_read_back(M.read_back_3x3(out, sites, 128), deq, bias)
