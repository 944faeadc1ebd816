"""The fixed-order reductions (colsum, db2_cone, dpos) and the patch-embed
data movement on non-square images, per element against fp64.

Integer probes in [-8, 8] keep every f32 partial sum an integer below 2^24,
so the result must equal the fp64 sum rounded once to bf16, in whatever
order the kernels add (``assert_exact``); random reals use ``gemm_tol`` with
K = the number of summands. The shapes visit the edges of the index
arithmetic: M around the 64-row chunk, the cap of 256 row chunks (where
trailing chunks are empty), the 16-way unroll of the finish (RB = 15, 16,
17), a second 8-wide column block (C = 2056 > 2048), the scalar path
(C = 588), and batch sizes below / not a multiple of dpos's 8 chunks.
"""

import pytest
import torch

from _bounds_util import assert_exact, assert_within, int_probe
from _stream_util import BF, colsum_ref, db2_ref, dpos_ref, nan_like

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"

# RB = 1, 1, 1, 2, 15, 16, 17, then 256 twice with empty trailing chunks
COLSUM_M = [1, 63, 64, 65, 960, 1024, 1025, 16385, 16384 + 130]
COLSUM_C = [8, 72, 588, 2056]
COLSUM_CASES = sorted({(M, 72) for M in COLSUM_M}
                      | {(1025, C) for C in COLSUM_C} | {(16385, 588)})


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@pytest.mark.parametrize("M,C", COLSUM_CASES)
def test_colsum(M, C):
    ext = _ext()
    g = _gen(M + C)
    x = int_probe((M, C), -8, 8, g)
    out = ext.colsum(x)
    assert out.shape == (C,)
    assert_exact(out, colsum_ref(x)[0], "colsum int")
    xr = torch.randn(M, C, device=DEV, generator=g).to(BF)
    ref, tol = colsum_ref(xr)
    print("colsum (%d, %d) err/tol %.3f"
          % (M, C, assert_within(ext.colsum(xr), ref, tol, "colsum randn")))


@pytest.mark.parametrize("shape", [(1, 9, 2, 8), (2, 33, 3, 24),
                                   (2, 16, 6, 512)], ids=str)
def test_db2_cone(shape):
    """Both outputs for every lo: fp64 column sums of the live columns, +0
    bits in the dead ones, whose input holds NaNs."""
    ext = _ext()
    B, N, L, d = shape
    g = _gen(5 + d)
    xi = int_probe(shape, -8, 8, g)
    xr = torch.randn(shape, device=DEV, generator=g).to(BF)
    worst = 0.0
    for lo in range(L + 1):
        for x in (xi, xr):
            p = x.clone()
            p[:, :, :lo] = nan_like(p[:, :, :lo])
            bu64, td64, tol = db2_ref(p, lo)
            bu, td = ext.db2_cone(p, lo)
            assert bu.shape == (L * d,) and td.shape == ((L - 1) * d,)
            if x is xi:
                assert_exact(bu, bu64, "dB2 bu lo=%d" % lo)
                assert_exact(td, td64, "dB2 td lo=%d" % lo)
            else:
                worst = max(worst,
                            assert_within(bu, bu64, tol, "dB2 bu lo=%d" % lo),
                            assert_within(td, td64, tol[:(L - 1) * d],
                                          "dB2 td lo=%d" % lo))
            assert not bu[:lo * d].view(torch.int16).any()
            assert not td[:lo * d].view(torch.int16).any()
    print("db2_cone %s err/tol %.3f" % (shape, worst))


@pytest.mark.parametrize("d", [8, 12, 72, 2056])
@pytest.mark.parametrize("B", [1, 3, 8, 9, 17])
def test_dpos(B, d):
    """Every l0 in 1..L for N in {1, 9}, L in {2, 3}; l0 = L gives all +0.
    The levels below l0 hold NaNs. d = 12 is accepted by the binding and
    runs the scalar kernel (no workspace is handed over when d % 8 != 0)."""
    ext = _ext()
    worst = 0.0
    for N in (1, 9):
        for L in (2, 3):
            g = _gen(B + N + L + d)
            xi = int_probe((B, N, L, d), -8, 8, g)
            xr = torch.randn(B, N, L, d, device=DEV, generator=g).to(BF)
            for l0 in range(1, L + 1):
                for x in (xi, xr):
                    p = x.clone()
                    p[:, :, :l0] = nan_like(p[:, :, :l0])
                    ref, tol = dpos_ref(p, l0)
                    got = ext.dpos(p, l0)
                    what = "dpos N=%d L=%d l0=%d" % (N, L, l0)
                    assert got.shape == (N, d)
                    if x is xi:
                        assert_exact(got, ref, what)
                    else:
                        worst = max(worst,
                                    assert_within(got, ref, tol, what))
                    if l0 == L:
                        assert not got.view(torch.int16).any()
    print("dpos B=%d d=%d err/tol %.3f" % (B, d, worst))


@pytest.mark.parametrize("H,W,P,dim", [(16, 24, 8, 64), (28, 42, 14, 64)])
def test_patch_embed_non_square(H, W, P, dim):
    """k_patchify / k_unpatchify compute with both H / P and W / P; integer
    probes make out, dW, db and dimg exact (K0 = 588 is padded to 640 for
    the second shape; every sum stays far below 2^24)."""
    from einops import rearrange
    from glom_pytorch_amd.ops.functional import PatchEmbedFn
    g = _gen(H + W)
    Bn = 3
    img = int_probe((Bn, 3, H, W), -4, 4, g)
    w = int_probe((dim, P * P * 3), -2, 2, g)
    b = int_probe((dim,), -8, 8, g)
    h, wp = H // P, W // P
    dY = int_probe((Bn, h * wp, dim), -2, 2, g)

    ig, wg, bg = (t.clone().requires_grad_(True) for t in (img, w, b))
    out = PatchEmbedFn.apply(ig, wg, bg, P)
    out.backward(dY)

    x64 = rearrange(img.double(), "b c (h p1) (w p2) -> b (h w) (p1 p2 c)",
                    p1=P, p2=P)
    assert x64.shape == (Bn, h * wp, P * P * 3)
    w64, b64, dy64 = w.double(), b.double(), dY.double()
    assert_exact(out, x64 @ w64.t() + b64, "out")
    M = Bn * h * wp
    assert_exact(wg.grad, dy64.reshape(M, dim).t() @ x64.reshape(M, -1), "dW")
    assert_exact(bg.grad, dy64.reshape(M, dim).sum(0), "db")
    dimg64 = rearrange(dy64 @ w64, "b (h w) (p1 p2 c) -> b c (h p1) (w p2)",
                       h=h, w=wp, p1=P, p2=P)
    assert_exact(ig.grad, dimg64, "dimg")
