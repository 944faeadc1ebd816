"""GELU and GELU' on every bf16 input, through the ops that apply them.

All 65,536 bf16 bit patterns are placed into the (1024 x 64) block of w1
(the 256 NaN / Inf patterns, exponent all ones, replaced by 0 and nothing
else). With one-hot token rows and zero bias the up-projection reproduces
them: Hpre[m, h] = w1[h, m % 64] exactly, so every finite bf16 value goes
through the GELU of whichever kernel serves the shape:

  k_gelu      (1, 64, 1, 64)    M = 64: generic GEMM, standalone GELU pass
  generic     (2, 256, 1, 72)   K = 72: generic kernel's EPI_GELU_PAIR
  nt4         (2, 256, 1, 64)   128 x 256 ring kernel's EPI_GELU_PAIR
  nt5p        (8, 256, 6, 64)   persistent ring: EPI_GELU_PAIR, and EPI_GELU
                                with save_for_bwd=False

Contract for Hact against the fp64 erf-GELU of the kernel's own Hpre:
  (a) |err| <= 2^-7 * |ref| + 3e-3. ops/csrc/common.h promises
      "matching nn.GELU() default within bf16 rounding": one bf16 ulp,
      2^-7 relative. The floor is the erf polynomial's stated accuracy,
      "~1e-3 abs", times the largest |d gelu / d erf| = 0.5 * |x| on the
      unclamped range |x / sqrt 2| <= 4: 0.5 * 4 * sqrt(2) * 1e-3 = 2.8e-3.
  (b) x < 0 never gives a result > 0.
  (c) x <= -8 gives exactly zero (of either sign).

GELU' goes through ff_bwd_dh: dH = acc * gelu'(Hpre) with an integer
acc = dY @ w2 (exact in f32) and the same swept Hpre. Bound:
|dH - acc * g'(x)| <= |acc| * 1e-3 + u * |ref|: the header's stated "~1e-3
abs" for the derivative polynomial, scaled by the exact factor, plus the one
bf16 rounding of the result (u = 2^-8; the rounded value is within u of the
f32 product, whose distance from ref the first term covers).
"""

import functools
import math

import pytest
import torch

from _bounds_util import U, assert_within, int_probe

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"
BF = torch.bfloat16
M4 = 1024

# name -> (B, N, L, d); bottom-up mode, G = L groups
FWD_CASES = {
    "k_gelu": (1, 64, 1, 64),
    "generic": (2, 256, 1, 72),
    "nt4": (2, 256, 1, 64),
    "nt5p": (8, 256, 6, 64),
}


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


@functools.lru_cache(maxsize=None)
def _patterns():
    """(1024, 64) bf16: every bit pattern once, NaN / Inf replaced by 0."""
    bits = torch.arange(-32768, 32768, dtype=torch.int32, device=DEV)
    nonfinite = (bits & 0x7F80) == 0x7F80
    assert int(nonfinite.sum()) == 256
    bits = torch.where(nonfinite, torch.zeros_like(bits), bits)
    pat = bits.to(torch.int16).view(BF).reshape(M4, 64)
    assert torch.isfinite(pat.float()).all()
    assert pat.view(torch.int16).unique().numel() == 65536 - 256
    return pat


def _gelu64(x):
    return 0.5 * x * (1 + torch.special.erf(x / math.sqrt(2)))


def _gelu_grad64(x):
    return (0.5 * (1 + torch.special.erf(x / math.sqrt(2)))
            + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi))


def _check_gelu(Hact, x, what):
    assert Hact.shape == x.shape
    ref = _gelu64(x)
    worst = assert_within(Hact, ref, 2.0 ** -7 * ref.abs() + 3e-3,
                          what + " (a)")
    h = Hact.double()
    npos = int(((x < 0) & (h > 0)).sum())
    assert npos == 0, "%s (b): %d negative inputs give a positive result, " \
        "largest %g" % (what, npos, h[x < 0].max().item())
    ntail = int(((x <= -8) & (h != 0)).sum())
    assert ntail == 0, "%s (c): %d inputs <= -8 give a nonzero result, " \
        "largest |.| %g" % (what, ntail, h[x <= -8].abs().max().item())
    print("gelu %s: worst err/tol %.3f" % (what, worst))


def _fwd_problem(B, N, L, d):
    """One-hot rows (group g hot at (m + g) % d), the swept w1 block in the
    first 64 columns of every group, zero biases; the expected Hpre."""
    M, G = B * N, L
    pat = _patterns()
    w1 = torch.zeros(G, M4, d, device=DEV, dtype=BF)
    w1[:, :, :64] = pat
    m = torch.arange(M, device=DEV)
    xs = torch.zeros(G, M, d, device=DEV, dtype=BF)
    for g in range(G):
        xs[g, m, (m + g) % d] = 1
    tokens = xs[0].reshape(B, N, d).contiguous()
    levels = torch.zeros(B, N, L, d, device=DEV, dtype=BF)
    for g in range(1, G):
        levels[:, :, g - 1] = xs[g].reshape(B, N, d)
    b1 = torch.zeros(G * M4, device=DEV, dtype=BF)
    w2 = torch.zeros(G * d, M4, device=DEV, dtype=BF)
    b2 = torch.zeros(G * d, device=DEV, dtype=BF)
    want = torch.matmul(xs.double(), w1.double().transpose(1, 2))
    # every group sees every finite bf16 value
    for g in range(G):
        assert want[g].unique().numel() == 65536 - 256 - 1   # -0 == +0
    return tokens, levels, w1.reshape(G * M4, d), b1, w2, b2, want


@pytest.mark.parametrize("name", list(FWD_CASES))
def test_gelu_all_bf16_inputs(name):
    B, N, L, d = FWD_CASES[name]
    tokens, levels, w1, b1, w2, b2, want = _fwd_problem(B, N, L, d)
    ext = _ext()
    _, Hpre, Hact, _ = ext.grouped_ff_fwd(tokens, levels, None, w1, b1, w2,
                                          b2, 0)
    assert torch.equal(Hpre.double(), want), "Hpre is not the swept block"
    _check_gelu(Hact, want, name)
    if name == "nt5p":
        _, Hpre2, Hact2, _ = ext.grouped_ff_fwd(tokens, levels, None, w1, b1,
                                                w2, b2, 0, False)
        assert Hpre2.numel() == 0
        _check_gelu(Hact2, want, name + " EPI_GELU")


@pytest.mark.parametrize("B,N,G", [(1, 64, 1), (8, 256, 6)],
                         ids=["generic", "nt5p"])
def test_gelu_grad_all_bf16_inputs(B, N, G):
    d, M = 64, B * N
    g = torch.Generator(device=DEV).manual_seed(B + G)
    dY = int_probe((B, N, G, d), -2, 2, g)
    w2t = int_probe((G, M4, d), -2, 2, g)
    pat = _patterns()
    m = torch.arange(M, device=DEV)
    Hpre = torch.stack([pat[:, (m + k) % 64].t() for k in range(G)])
    Hpre = Hpre.contiguous()                                  # (G, M, M4)
    dH, _ = _ext().ff_bwd_dh(dY, w2t, Hpre)
    acc = torch.matmul(dY.double().permute(2, 0, 1, 3).reshape(G, M, d),
                       w2t.double().transpose(1, 2))          # integers
    assert float(acc.abs().max()) <= 256
    ref = acc * _gelu_grad64(Hpre.double())
    worst = assert_within(dH, ref, acc.abs() * 1e-3 + U * ref.abs(),
                          "gelu' through ff_bwd_dh")
    print("gelu' %s: worst err/tol %.3f" % ((B, N, G), worst))
