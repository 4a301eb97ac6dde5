"""Exact index and key-count tests for every dispatch branch of the attention kernels (srgd_amd/csrc/attention.hip), through
the kernel-level C ABI.  The inputs and their closed-form outputs come from tests/attention_cases.py (proven against the float64
oracle in tests/test_attention_cases_cpu.py):

  A  full attention, one-hot by a random permutation, logits up to 1448: out[i] = v[pi(i)] bit for bit
  B  full attention, q = 0: out = sum of integer v over all keys / N (bit-exact for N = 2^k, else 2^-21 / 2^-8 relative)
  C  linear attention, one-hot k per channel and q per position, spikes on every chunk seam: out = fl32(v * 1/sqrt(32)) bit for bit
  D  linear attention, k = 0: out = sum of integer v over all positions / sqrt(32) / N (tolerances as in B)
  G  Gaussian data with the spikes of test_{full,linear}_attention_core, against the float64 oracle, within tol()

The output buffer is pre-filled with NaN, so a row the kernel never wrote fails too.  Every case appends its max error to
the parity report of tests/test_kernels_gpu.py (`_report_k`)."""
import pytest
import torch

from oracle import srgd_oracle as O
from tests import attention_cases as AC
from tests.test_kernels_gpu import DEV, L, _report_k, from_dev_nhwc, ptr, rnd, stream, to_dev_nhwc, tol

pytestmark = pytest.mark.gpu


def run_attention(which, qkv, heads, bf16):
    lib = L().lib()
    B, _, H, W = qkv.shape
    d = to_dev_nhwc(qkv, bf16)
    out = torch.full((B, H, W, heads * 32), float("nan"), device=DEV, dtype=d.dtype)
    fn = lib.srgd_k_full_attention if which == "full" else lib.srgd_k_linear_attention
    L().check(fn(ptr(d), ptr(out), B, H * W, heads, int(bf16), stream()), which + " attention")
    torch.cuda.synchronize()
    return from_dev_nhwc(out)


def _check_case(which, construction, shape, case):
    group, elem, B, heads, n = shape
    bf16 = elem == "bf16"
    got = run_attention(which, case.qkv, heads, bf16)
    rec = dict(test="attention_exact", construction=construction, group=group, elem=elem, B=B, heads=heads, N=n,
               exact=case.exact)
    try:
        err = AC.assert_matches(case, got, bf16)
    except AssertionError:
        want = AC.bf16_round(case.want) if bf16 and case.exact else case.want
        _report_k(**rec, max_err=float((got.double() - want.double()).abs().max()), passed=False)
        raise
    print("%s %s: max |err| = %.3e" % (construction, AC.shape_id(shape), err))
    _report_k(**rec, max_err=err, passed=True)


def _check_gaussian(which, shape, qkv):
    group, elem, B, heads, n = shape
    bf16 = elem == "bf16"
    qkv = rnd(qkv, bf16)
    got = run_attention(which, qkv, heads, bf16)
    core = O.full_attention_core if which == "full" else O.linear_attention_core
    want = core(qkv.double(), heads, 32)
    err = float((got.double() - want).abs().max())
    bound = tol(bf16, want)
    print("G %s: max |err| = %.3e (bound %.3e)" % (AC.shape_id(shape), err, bound))
    _report_k(test="attention_exact", construction="G", group=group, elem=elem, B=B, heads=heads, N=n, exact=False,
              max_err=err, bound=bound, passed=bool(err <= bound))
    assert err <= bound, (err, bound)                                      # NaN compares false


@pytest.mark.parametrize("shape", AC.FULL_SHAPES, ids=AC.shape_id)
def test_full_attention_permutation_is_bit_exact(shape):
    _, _, B, heads, n = shape
    case = AC.full_permutation(B, heads, n)
    assert case.exact
    _check_case("full", "A", shape, case)


@pytest.mark.parametrize("shape", AC.FULL_SHAPES, ids=AC.shape_id)
def test_full_attention_uniform_counts_every_key_once(shape):
    _, elem, B, heads, n = shape
    case = AC.full_uniform(B, heads, n, AC.cap_of(elem))
    assert case.meta["smax"] <= AC.cap_of(elem)
    _check_case("full", "B", shape, case)


@pytest.mark.parametrize("shape", AC.FULL_SHAPES, ids=AC.shape_id)
def test_full_attention_gaussian_against_float64(shape):
    _, _, B, heads, n = shape
    _check_gaussian("full", shape, AC.gaussian_full(B, heads, n))


@pytest.mark.parametrize("shape", AC.LINEAR_SHAPES, ids=AC.shape_id)
def test_linear_attention_selection_is_bit_exact(shape):
    _, _, B, heads, n = shape
    case = AC.linear_selection(B, heads, n)
    assert case.exact
    _check_case("linear", "C", shape, case)


@pytest.mark.parametrize("shape", AC.LINEAR_SHAPES, ids=AC.shape_id)
def test_linear_attention_uniform_counts_every_position_once(shape):
    _, elem, B, heads, n = shape
    case = AC.linear_uniform(B, heads, n, AC.cap_of(elem))
    assert case.meta["smax"] <= AC.cap_of(elem)
    _check_case("linear", "D", shape, case)


@pytest.mark.parametrize("shape", AC.LINEAR_SHAPES, ids=AC.shape_id)
def test_linear_attention_gaussian_against_float64(shape):
    _, _, B, heads, n = shape
    _check_gaussian("linear", shape, AC.gaussian_linear(B, heads, n))
