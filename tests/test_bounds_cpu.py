"""The per-element checker (tests/_bounds_util.py), tested on the CPU.

A CPU emulation of the GEMM kernels' contract (bf16 operands, f32
accumulate, bias in f32, one bf16 rounding) must pass both asserts; each of
a set of small faults injected into that output must fail them. The faults
are the ones a whole-tensor relative-norm bound of 1.5e-2 lets through.
"""

import pytest
import torch

from _bounds_util import (U, assert_exact, assert_within, gemm_tol,
                          int_probe, round_once)

BF = torch.bfloat16

# (M, N, K); the fragment mutated below is rows 16..31, columns 32..47
RANDN_SHAPES = [(256, 512, 64), (256, 256, 2048), (130, 72, 200)]
INT_SHAPES = RANDN_SHAPES + [(256, 256, 8192)]


def _emulate(A, B, bias):
    return (A.float() @ B.float().t() + bias.float()).to(BF)


def _problem(M, N, K, integer):
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K + integer)
    if integer:
        A = int_probe((M, K), -2, 2, g)
        B = int_probe((N, K), -2, 2, g)
        bias = int_probe((N,), -8, 8, g)
    else:
        A = torch.randn(M, K, generator=g).to(BF)
        B = torch.randn(N, K, generator=g).to(BF)
        bias = torch.randn(N, generator=g).to(BF)
    ref = A.double() @ B.double().t() + bias.double()
    absprod = A.double().abs() @ B.double().abs().t() + bias.double().abs()
    return A, B, bias, ref, absprod


def _mut_ktail(out, A, B, bias):
    o = out.clone()
    K = A.shape[1]
    o[16:32, 32:48] = _emulate(A[16:32, :K - 8], B[32:48, :K - 8],
                               bias[32:48])
    return o


def _mut_rows(out, A, B, bias):
    o = out.clone()
    o[[3, 77]] = out[[77, 3]]
    return o


def _mut_bias(out, A, B, bias):
    o = out.clone()
    j = int(bias.float().abs().argmax())     # a column whose bias is not 0
    o[:, j] = _emulate(A, B[j:j + 1], torch.zeros(1, dtype=BF))[:, 0]
    return o


def _mut_transpose(out, A, B, bias):
    o = out.clone()
    o[16:32, 32:48] = out[16:32, 32:48].t()
    return o


def _mut_ulps(out, A, B, bias):
    o = out.clone()
    bits = o.view(torch.int16)
    bits[40, 9] += 2
    return o


MUTATIONS = [_mut_ktail, _mut_rows, _mut_bias, _mut_transpose]


def test_round_once_beats_double_rounding():
    # 1 + 2^-8 + 2^-30 lies just above the tie between 1 and 1 + 2^-7:
    # rounding through fp32 first lands on the tie and then on the even
    # neighbour 1.0; a single rounding gives 1 + 2^-7
    x = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -30, -(1 + 2.0 ** -8 + 2.0 ** -30),
                      1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 0.0, 3.0],
                     dtype=torch.float64)
    want = torch.tensor([1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1.0,
                         1 + 2.0 ** -6, 0.0, 3.0], dtype=torch.float64)
    assert torch.equal(round_once(x, BF).double(), want)
    assert x.float().to(BF)[0].item() == 1.0      # what torch alone does
    assert torch.equal(round_once(x, torch.float32), x.float())


@pytest.mark.parametrize("M,N,K", INT_SHAPES)
def test_integer_probe_exact(M, N, K):
    A, B, bias, ref, absprod = _problem(M, N, K, True)
    out = _emulate(A, B, bias)
    assert_exact(out, ref)
    assert_within(out, ref, gemm_tol(ref, absprod, K))
    # every partial sum is an integer below 2^24: order cannot matter
    assert float(absprod.max()) < 2 ** 24
    assert_exact(_emulate(A.flip(1), B.flip(1), bias), ref)
    for mut in MUTATIONS + [_mut_ulps]:
        with pytest.raises(AssertionError, match="differ"):
            assert_exact(mut(out, A, B, bias), ref, mut.__name__)


@pytest.mark.parametrize("M,N,K", RANDN_SHAPES)
def test_randn_within_gemm_tol(M, N, K):
    A, B, bias, ref, absprod = _problem(M, N, K, False)
    out = _emulate(A, B, bias)
    tol = gemm_tol(ref, absprod, K)
    worst = assert_within(out, ref, tol)
    assert 0 < worst <= 1
    for mut in MUTATIONS:
        with pytest.raises(AssertionError, match="out of tolerance"):
            assert_within(mut(out, A, B, bias), ref, tol, mut.__name__)


def test_ktail_mutation_flips_most_of_the_fragment():
    A, B, bias, ref, _ = _problem(256, 256, 8192, True)
    bad = _mut_ktail(_emulate(A, B, bias), A, B, bias)
    want = round_once(ref, BF)
    n = int((bad != want).sum())
    assert 200 <= n <= 256, n


def test_assert_within_excludes_nothing():
    ref = torch.zeros(4, 4, dtype=torch.float64)
    out = torch.zeros(4, 4, dtype=BF)
    assert assert_within(out, ref, 0.0) == 0.0
    for v in (float("nan"), float("inf"), 2.0 ** -100):
        o = out.clone()
        o[2, 3] = v
        with pytest.raises(AssertionError, match=r"1 of 16 .*\(2, 3\)"):
            assert_within(o, ref, 1e-40)


def test_assert_exact_reports_index_and_fp32():
    ref = torch.arange(12, dtype=torch.float64).reshape(3, 4) / 3
    assert_exact(ref.float(), ref)
    o = round_once(ref, BF)
    assert_exact(o, ref)
    o[1, 2] = 7
    with pytest.raises(AssertionError, match=r"1 of 12 .*\(1, 2\), 7\.0"):
        assert_exact(o, ref)
    z = torch.zeros(2, dtype=BF)
    with pytest.raises(AssertionError):          # -0 is not +0 bit for bit
        assert_exact(-z, torch.zeros(2, dtype=torch.float64))


def test_gemm_tol_formula():
    ref = torch.tensor([4.0, -2.0], dtype=torch.float64)
    ap = torch.tensor([8.0, 2.0], dtype=torch.float64)
    t = gemm_tol(ref, ap, 61)
    want = U * ref.abs() + (1 + U) * 64 * 2.0 ** -23 * ap
    assert torch.equal(t, want)
