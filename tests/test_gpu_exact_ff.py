"""The grouped feed-forward ops through their real entry points, bit-exact
on integer probes: grouped_ff_fwd, ff_bwd_dh, ff_bwd_dx, ff_bwd_dw and
grouped_ff_bwd, bottom-up (mode 0) and top-down (mode 1).

The GEMM stages (Hpre, Y, td_in, dX, dW1, dW2, dB1, dB2) see only integers,
so f32 accumulation is exact in any order and every output must equal the
fp64 result rounded once to bf16 (tests/_bounds_util.py): that covers the
table-resolved / strided operand reads, the table-scattered dX, the split
into live and dead groups (g_lo, group0_done) and the zero-filled slices.

GELU and GELU' sit between those stages; test_gpu_gelu_sweep.py holds them
to their own contract. Here they are kept out of the way by probing them
only where they are exact:
  * w1 and b1 are multiples of 8, so Hpre is 0 or |Hpre| >= 8, where
    gelu(x) is exactly 0 or x (erf saturated, the result clamped to the
    interval between 0 and x): the returned Hact is integer-valued and Y,
    recomputed from it, is exact;
  * the backward gets Hpre = 0, where gelu'(0) = 0.5 + 0 * P(0) = 0.5
    exactly, and an even dY, so dHpre = (dY @ w2) / 2 is an integer.

Magnitudes: |x| <= 2 (+ pos <= 2), |w1| <= 16, |b1| <= 64, |w2| <= 2,
|dY| <= 4, d = 64, m4 <= 1024, M <= 2048. |Hpre| <= 4*16*64 + 64 = 4160,
|Y| <= 1024 * 4160 * 2 + 8 < 2^24, |dHpre| <= 64*4*2/2 = 256 (exact in
bf16, so the fused dB1, summed before the rounding, and the standalone one,
summed after it, see the same values), every other sum is smaller.
"""

import functools

import pytest
import torch

from _bounds_util import assert_exact, int_probe

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"
BF = torch.bfloat16

SMALL = (2, 16, 3, 64, 256)       # generic kernels, standalone colsum
LARGE = (8, 256, 6, 64, 1024)     # nt5p: EPI_GELU_PAIR / EPI_GELU, fused dB1
CASES = [SMALL, LARGE]


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


class _Problem:
    pass


@functools.lru_cache(maxsize=2)
def _problem(case, mode):
    B, N, L, d, m4 = case
    G = L if mode == 0 else L - 1
    M = B * N
    g = torch.Generator(device=DEV).manual_seed(17 * M + m4 + mode)
    p = _Problem()
    p.B, p.N, p.L, p.d, p.m4, p.G, p.M, p.mode = B, N, L, d, m4, G, M, mode
    p.tokens = int_probe((B, N, d), -2, 2, g) if mode == 0 else None
    p.levels = int_probe((B, N, L, d), -2, 2, g)
    p.pos = int_probe((N, d), -2, 2, g) if mode == 1 else None
    p.w1 = int_probe((G * m4, d), -2, 2, g) * 8
    p.b1 = int_probe((G * m4,), -8, 8, g) * 8
    p.w2 = int_probe((G * d, m4), -2, 2, g)
    p.b2 = int_probe((G * d,), -8, 8, g)
    p.dY = int_probe((B, N, G, d), -2, 2, g) * 2
    p.dH = int_probe((G, M, m4), -2, 2, g)        # an integer dHpre
    p.Hact = int_probe((G, M, m4), -2, 2, g)      # an integer activation
    p.w1t = p.w1.view(G, m4, d).transpose(1, 2).contiguous()
    p.w2t = p.w2.view(G, d, m4).transpose(1, 2).contiguous()
    lv = p.levels.double()
    if mode == 0:
        xs = [p.tokens.double().reshape(M, d)] + [
            lv[:, :, k].reshape(M, d) for k in range(L - 1)]
    else:
        p.td_ref = lv[:, :, 1:] + p.pos.double().view(1, N, 1, d)
        xs = [p.td_ref[:, :, k].reshape(M, d) for k in range(G)]
    p.x = torch.stack(xs)                                     # (G, M, d)
    p.w1g = p.w1.double().view(G, m4, d)
    p.w2g = p.w2.double().view(G, d, m4)
    p.hpre_ref = (torch.matmul(p.x, p.w1g.transpose(1, 2))
                  + p.b1.double().view(G, 1, m4))
    return p


def _y_ref(p, Hact):
    y = (torch.matmul(Hact.double(), p.w2g.transpose(1, 2))
         + p.b2.double().view(p.G, 1, p.d))                   # (G, M, d)
    return y.permute(1, 0, 2).reshape(p.B, p.N, p.G, p.d)


def _live(p, t, g_lo):
    """`t` (G, ...) with the dead groups [0, g_lo) replaced by zeros."""
    t = t.clone()
    t[:g_lo] = 0
    return t


def _dy(p, g_lo):
    dY = p.dY.clone()
    dY[:, :, :g_lo] = 0          # the level-cone promise
    return dY


def _dx_ref(p, dH64, g_lo):
    """(dTokens, dLevels) from an fp64 dHpre whose dead groups are zero."""
    dx = torch.matmul(dH64, p.w1g)                            # (G, M, d)
    dx = _live(p, dx, g_lo).view(p.G, p.B, p.N, p.d)
    dlev = torch.zeros(p.B, p.N, p.L, p.d, dtype=torch.float64, device=DEV)
    if p.mode == 0:
        for k in range(1, p.G):
            dlev[:, :, k - 1] = dx[k]
        return dx[0], dlev
    for k in range(p.G):
        dlev[:, :, k + 1] = dx[k]
    return None, dlev


def _dw_ref(p, dY, dH64, Hact, g_lo):
    dyg = dY.double().permute(2, 0, 1, 3).reshape(p.G, p.M, p.d)
    dW1 = _live(p, torch.matmul(dH64.transpose(1, 2), p.x), g_lo)
    dW2 = _live(p, torch.matmul(dyg.transpose(1, 2), Hact.double()), g_lo)
    dB2 = dY.double().reshape(p.M, p.G * p.d).sum(0)
    return (dW1.reshape(p.G * p.m4, p.d), dW2.reshape(p.G * p.d, p.m4), dB2)


def _dh_ref(p, dY, g_lo):
    """dHpre at Hpre = 0: (dY_g @ w2_g) * 0.5, dead groups zero."""
    dyg = dY.double().permute(2, 0, 1, 3).reshape(p.G, p.M, p.d)
    return _live(p, torch.matmul(dyg, p.w2g) * 0.5, g_lo)


def _g_los(case, mode):
    G = case[2] if mode == 0 else case[2] - 1
    return sorted({0, 1, G - 1}) if case == SMALL else [0]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=["small", "large"])
def test_ff_fwd_exact(case, mode):
    p = _problem(case, mode)
    ext = _ext()
    Y, Hpre, Hact, td_in = ext.grouped_ff_fwd(
        p.tokens, p.levels, p.pos, p.w1, p.b1, p.w2, p.b2, mode)
    assert_exact(Hpre, p.hpre_ref, "Hpre")
    assert Hact.shape == Hpre.shape
    assert_exact(Y, _y_ref(p, Hact), "Y")
    if mode == 1:
        assert_exact(td_in, p.td_ref, "td_in")
    # forward-only call: EPI_GELU on the nt5p shape, no Hpre at all
    Y2, Hpre2, Hact2, _ = ext.grouped_ff_fwd(
        p.tokens, p.levels, p.pos, p.w1, p.b1, p.w2, p.b2, mode, False)
    assert Hpre2.numel() == 0
    assert torch.equal(Hact2, Hact)
    assert_exact(Y2, _y_ref(p, Hact2), "Y (forward-only)")


def test_ff_fwd_group0_done_exact():
    p = _problem(SMALL, 0)
    Y, Hpre, Hact, _ = _ext().grouped_ff_fwd(
        p.tokens, p.levels, None, p.w1, p.b1, p.w2, p.b2, 0, True, True)
    assert_exact(Hpre[1:], p.hpre_ref[1:], "Hpre[1:]")
    Hact = Hact.clone()
    Hact[0] = 0                  # left unwritten, like Y[:, :, 0]
    assert_exact(Y[:, :, 1:], _y_ref(p, Hact)[:, :, 1:], "Y[:, :, 1:]")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=["small", "large"])
def test_ff_bwd_stages_exact(case, mode):
    p = _problem(case, mode)
    ext = _ext()
    zeros = torch.zeros(p.G, p.M, p.m4, device=DEV, dtype=BF)
    for g_lo in _g_los(case, mode):
        tag = "g_lo=%d " % g_lo
        dY = _dy(p, g_lo)
        # dH at Hpre = 0, with dB1 (fused on the large case)
        dHpre, dB1 = ext.ff_bwd_dh(dY, p.w2t, zeros, g_lo)
        dh_ref = _dh_ref(p, dY, g_lo)
        assert_exact(dHpre[g_lo:], dh_ref[g_lo:], tag + "dHpre")
        assert_exact(dB1, dh_ref.sum(1).reshape(-1), tag + "dB1")
        # dX from an integer dHpre (its dead groups are never read)
        dTok, dLev = ext.ff_bwd_dx(p.dH, p.w1t, p.tokens, p.B, p.N, p.L,
                                   mode, g_lo)
        rTok, rLev = _dx_ref(p, p.dH.double(), g_lo)
        assert_exact(dLev, rLev, tag + "dLevels")
        if mode == 0:
            assert_exact(dTok, rTok, tag + "dTokens")
        # dW1, dW2, dB2 from integer dHpre and Hact
        dW1, dW2, dB2 = ext.ff_bwd_dw(dY, p.dH, p.tokens, p.levels, p.pos,
                                      p.Hact, mode, None, g_lo)
        r1, r2, rb = _dw_ref(p, dY, p.dH.double(), p.Hact, g_lo)
        assert_exact(dW1, r1, tag + "dW1")
        assert_exact(dW2, r2, tag + "dW2")
        assert_exact(dB2, rb, tag + "dB2")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=["small", "large"])
def test_grouped_ff_bwd_exact(case, mode):
    p = _problem(case, mode)
    ext = _ext()
    zeros = torch.zeros(p.G, p.M, p.m4, device=DEV, dtype=BF)
    for g_lo in _g_los(case, mode):
        tag = "g_lo=%d " % g_lo
        dY = _dy(p, g_lo)
        dTok, dLev, dW1, dB1, dW2, dB2 = ext.grouped_ff_bwd(
            dY, p.tokens, p.levels, p.pos, p.w1, p.w2, zeros, p.Hact, mode,
            None, None, None, g_lo)
        dh = _dh_ref(p, dY, g_lo)          # integers <= 256: exact in bf16
        assert float(dh.abs().max()) <= 256
        rTok, rLev = _dx_ref(p, dh, g_lo)
        r1, r2, rb = _dw_ref(p, dY, dh, p.Hact, g_lo)
        assert_exact(dLev, rLev, tag + "dLevels")
        if mode == 0:
            assert_exact(dTok, rTok, tag + "dTokens")
        assert_exact(dW1, r1, tag + "dW1")
        assert_exact(dB1, dh.sum(1).reshape(-1), tag + "dB1")
        assert_exact(dW2, r2, tag + "dW2")
        assert_exact(dB2, rb, tag + "dB2")
