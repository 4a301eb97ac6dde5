"""The closed-form attention cases of tests/attention_cases.py, proven on the CPU: every construction equals the float64
oracle, the stated |S_e| caps hold for every shape the GPU file runs, and the very assertion the GPU file uses rejects an
attention that drops one key, counts one twice or pairs two keys with each other's V rows."""
import pytest
import torch

from oracle import srgd_oracle as O
from tests import attention_cases as AC


def _close(got, want, rel):
    return bool(((got.double() - want.double()).abs() <= rel * want.double().abs()).all())


# ------------------------------------------------------------------ each construction equals the oracle
@pytest.mark.parametrize("shape", [(3, 1, 17), (2, 4, 99), (1, 4, 256), (1, 2, 1024), (1, 1, 4096)], ids=lambda s: "B%d_h%d_N%d" % s)
def test_permutation_case_is_exactly_the_oracle(shape):
    B, heads, n = shape
    c = AC.full_permutation(B, heads, n)
    assert torch.equal(O.full_attention_core(c.qkv.double(), heads, 32), c.want.double())
    assert torch.equal(O.full_attention_core(c.qkv, heads, 32), c.want)
    assert torch.equal(AC.bf16_round(c.qkv), c.qkv)                     # the same tensor serves bf16 mode
    bits, reps, a = AC.permutation_code(n)
    u = AC.key_codes(n)
    if n > 1:                                                           # the lead the construction promises, from the codes themselves
        gram = u @ u.t()
        gram.fill_diagonal_(-1e9)
        assert float(a * (32 - gram.max()) / 32 ** 0.5) >= AC.LEAD
    assert a == {17: 64, 99: 128, 256: 128, 1024: 128, 4096: 256}[n]


@pytest.mark.parametrize("shape", [(2, 4, 99, 64), (1, 8, 256, 64), (1, 4, 1000, 4096), (2, 1, 1280, 64), (1, 2, 4096, 64), (1, 1, 4096, 4096)],
                         ids=lambda s: "B%d_h%d_N%d_cap%d" % s)
def test_uniform_full_case_is_the_oracle(shape):
    B, heads, n, cap = shape
    c = AC.full_uniform(B, heads, n, cap)
    ref = O.full_attention_core(c.qkv.double(), heads, 32)
    assert float((ref - c.want.double()).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    assert c.exact == (n & (n - 1) == 0)
    assert torch.equal(AC.bf16_round(c.qkv), c.qkv)
    if c.exact:                                                         # bf16 output rounding leaves an exact case exact
        assert cap > 64 or torch.equal(AC.bf16_round(c.want), c.want)


@pytest.mark.parametrize("shape", [(3, 4, 4), (2, 1, 100), (2, 4, 960), (3, 8, 1023), (1, 4, 16448)], ids=lambda s: "B%d_h%d_N%d" % s)
def test_selection_case_is_the_oracle(shape):
    B, heads, n = shape
    c = AC.linear_selection(B, heads, n)
    # float64: equal up to the fp32 rounding of v * scale and of the scale itself
    assert _close(c.want, O.linear_attention_core(c.qkv.double(), heads, 32), 1.5 * 2.0 ** -23)
    # float32: the oracle's only rounding is that product, with the same fp32 scale the host computes -> bit-equal
    assert torch.equal(O.linear_attention_core(c.qkv, heads, 32), c.want)
    assert torch.equal(AC.bf16_round(c.qkv), c.qkv)
    p = c.meta["p"].flatten().tolist()
    for s in AC.seam_positions(n, B * heads * 32):                      # every seam position carries a spike
        assert s in p
    assert {0, n - 1} <= set(p)
    if n > 1024:
        assert {511, 512, 1023, 1024} <= set(p)


def test_selection_case_covers_all_1024_seams_at_the_production_length():
    pos = AC.seam_positions(65536, 1 * 4 * 32)
    assert set(pos) == {0, 65535} | {s + d for s in range(1024, 65536, 1024) for d in (-1, 0)}


@pytest.mark.parametrize("shape", [(2, 1, 100, 64), (1, 4, 512, 64), (3, 8, 1023, 4096), (1, 4, 16448, 64), (1, 4, 65536, 4096), (1, 4, 65536, 64)],
                         ids=lambda s: "B%d_h%d_N%d_cap%d" % s)
def test_uniform_linear_case_is_the_oracle(shape):
    B, heads, n, cap = shape
    c = AC.linear_uniform(B, heads, n, cap)
    ref = O.linear_attention_core(c.qkv.double(), heads, 32)
    if c.exact:                                                         # expectation holds the fp32 rounding of S_e * fl32(1/sqrt(32))
        assert _close(c.want, ref, 1.5 * 2.0 ** -23)
    else:
        assert float((ref - c.want).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    assert torch.equal(AC.bf16_round(c.qkv), c.qkv)


def test_slot_references_with_identity_slots_are_the_oracle():
    qf, ql = AC.gaussian_full(2, 4, 99), AC.gaussian_linear(2, 4, 100)
    assert torch.allclose(AC.full_attention_slots(qf, 4, list(range(99))), O.full_attention_core(qf.double(), 4, 32), rtol=0, atol=1e-13)
    assert torch.allclose(AC.linear_attention_slots(ql, 4, list(range(100))), O.linear_attention_core(ql.double(), 4, 32), rtol=0, atol=1e-13)


# ------------------------------------------------------------------ the caps, for every shape of the GPU file
@pytest.mark.parametrize("shape", AC.FULL_SHAPES + AC.LINEAR_SHAPES, ids=AC.shape_id)
def test_counting_weights_respect_the_cap(shape):
    _, elem, B, heads, n = shape
    cap = AC.cap_of(elem)
    w, layout = AC.counting_weights(n, cap)
    S = AC.channel_sums(w)
    assert int(S.max()) <= cap
    assert int(S.sum()) == int(w.sum()) and int(w.min()) >= 0
    rel = AC.REL_BF16 if elem == "bf16" else AC.REL_FP32
    assert 1.0 / int(S.max()) >= 4 * rel                                # one key of weight >= 1 moves its channel by >= 4 x the tolerance
    if layout != "sparse":
        assert int(w.min()) >= 1                                        # every key counted
    else:
        assert n > 32 * cap and {0, n - 1, 511, 512} <= set(w.nonzero().flatten().tolist())
    assert layout == ("w123" if n <= (1024 if elem == "bf16" else 65536) else "ones" if n <= 2048 else "sparse")


def test_shape_table_reaches_every_branch_with_the_required_batches_and_heads():
    for group, elem in [("scalar", "fp32"), ("scalar", "bf16"), ("mfma", "fp32"), ("mfma", "bf16"), ("lds", "bf16"),
                        ("linear", "fp32"), ("linear", "bf16")]:
        rows = [s for s in AC.FULL_SHAPES + AC.LINEAR_SHAPES if s[:2] == (group, elem)]
        assert {1, 3} <= {s[2] for s in rows} and {1, 8} <= {s[3] for s in rows}, (group, elem)
    for group, elem, B, heads, n in AC.FULL_SHAPES:                     # the dispatch of full_attention()
        want = "lds" if elem == "bf16" and n % 256 == 0 and n <= 1024 else "mfma" if n % 32 == 0 else "scalar"
        assert group == want, (group, elem, n)
    ns = lambda g, e: sorted(s[4] for s in AC.FULL_SHAPES + AC.LINEAR_SHAPES if s[:2] == (g, e))
    assert ns("scalar", "fp32") == ns("scalar", "bf16") == [1, 17, 99, 100, 1000]
    assert ns("mfma", "fp32") == [32, 96, 1024, 4096] and ns("mfma", "bf16") == [1280, 4096]
    assert ns("lds", "bf16") == [256, 512, 768, 1024]
    assert ns("linear", "fp32") == ns("linear", "bf16") == [4, 100, 512, 516, 1023, 16384, 16448, 65536]


# ------------------------------------------------------------------ mutation: a subtly wrong attention must fail the assertion
def _as_kernel_output(x, bf16):
    return AC.bf16_round(x.float()) if bf16 else x.float()


def _full_case(which, n, bf16):
    return AC.full_permutation(2, 4, n) if which == "A" else AC.full_uniform(2, 4, n, AC.cap_of("bf16" if bf16 else "fp32"))


def _linear_case(which, n, bf16):
    return AC.linear_selection(2, 4, n) if which == "C" else AC.linear_uniform(2, 4, n, AC.cap_of("bf16" if bf16 else "fp32"))


def _defect_at(c, which, n, defect):
    """Where the defect sits: the last key of the first 64-key tile / 512-position chunk where there is one (A, B, D), the
    spike position of a channel that some query reads (C); a sparse counting case can only notice a covered key."""
    if which == "C":
        j = int(c.meta["p"][0, 0, c.meta["dstar"][0, 0, 0]])
    else:
        j = min(n - 1, 511 if which == "D" else 63)
        if which in "BD":
            cov = c.meta["covered"]
            j = int(cov[cov <= j].max())
    return AC.defect_slots(n, defect, j, (j + 1) % n)


# which defect each construction must notice; the complementary pairs are test_each_kind_is_blind_where_the_other_sees
SEES = [("A", "drop"), ("A", "swap"), ("B", "drop"), ("B", "dup"), ("C", "drop"), ("C", "swap"), ("D", "drop"), ("D", "dup")]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [99, 1024, 1280, 4096])
@pytest.mark.parametrize("which,defect", [s for s in SEES if s[0] in "AB"])
def test_full_cases_reject_a_defective_attention(which, defect, n, bf16):
    c = _full_case(which, n, bf16)
    dt = torch.float32 if c.exact else torch.float64                       # an exact expectation holds fp32 roundings
    good = AC.full_attention_slots(c.qkv, 4, list(range(n)), dtype=dt)
    AC.assert_matches(c, _as_kernel_output(good, bf16), bf16)             # the intact reference passes ...
    bad = AC.full_attention_slots(c.qkv, 4, *_defect_at(c, which, n, defect), dtype=dt)
    with pytest.raises(AssertionError):                                    # ... the defective one does not
        AC.assert_matches(c, _as_kernel_output(bad, bf16), bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [100, 1023, 16384, 16448])
@pytest.mark.parametrize("which,defect", [s for s in SEES if s[0] in "CD"])
def test_linear_cases_reject_a_defective_attention(which, defect, n, bf16):
    c = _linear_case(which, n, bf16)
    dt = torch.float32 if c.exact else torch.float64
    good = AC.linear_attention_slots(c.qkv, 4, list(range(n)), dtype=dt)
    AC.assert_matches(c, _as_kernel_output(good, bf16), bf16)
    bad = AC.linear_attention_slots(c.qkv, 4, *_defect_at(c, which, n, defect), dtype=dt)
    with pytest.raises(AssertionError):
        AC.assert_matches(c, _as_kernel_output(bad, bf16), bf16)


def test_each_kind_is_blind_where_the_other_sees():
    # why both kinds exist: a key counted twice in numerator AND denominator leaves a one-hot softmax's output unchanged (A, C),
    # two V rows swapped leave a plain sum unchanged (B, D)
    for which, defect in [("A", "dup"), ("B", "swap")]:
        c = _full_case(which, 99, False)
        AC.assert_matches(c, AC.full_attention_slots(c.qkv, 4, *_defect_at(c, which, 99, defect)).float(), False)
        assert c.exact == (which == "A")
    for which, defect in [("C", "dup"), ("D", "swap")]:
        c = _linear_case(which, 1023, False)
        got = AC.linear_attention_slots(c.qkv, 4, *_defect_at(c, which, 1023, defect), dtype=torch.float32 if c.exact else torch.float64)
        AC.assert_matches(c, got.float(), False)


def test_assertion_rejects_nan_and_unwritten_output():
    for c in (AC.full_permutation(1, 1, 17), AC.full_uniform(1, 1, 17, 64)):
        got = c.want.float().clone()
        AC.assert_matches(c, got, False)
        got[0, 3, 0, 5] = float("nan")
        with pytest.raises(AssertionError):
            AC.assert_matches(c, got, False)
