"""TN GEMM with direct-to-LDS staging and transposed LDS reads (gemm_tn_tr)
and the re-blocked split-K finish (gemm_finish4).

Both keep every f32 operation of an output element in the same order as the
kernels they replace (same MFMA, same k -> lane-group map, ascending k, same
split-K partition, same finish order), so the requirement is bit equality
with set_tn_tr(False) / set_finish_wide(False) in the same process, plus
correctness against an fp64 product of the same bf16 inputs with the
relative-norm bound the GEMM sweep test uses for its TN products (5e-2,
tests/test_gpu_gemm_sweep.py).

Split-K (run_gemm): a TN call with fewer than 1024 128^2 tiles and
K >= 4096 is split min(16, 2048 / tiles, K / 64) ways; a slice covers
`per` = ceil(ceil(K/64) / split) * 64 rows of K.
"""

import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"
BF = torch.bfloat16
TN_BOUND = 5e-2

# (M, N, K, G) through ext.gemm_tn
GEMM_CASES = [
    (128, 128, 64, 1),     # non-split; one K-step: prologue = whole loop
    (128, 128, 192, 3),    # non-split; odd step count, buffer parity
    (256, 128, 4096, 1),   # split-K 16, 4 steps per slice; two M-tiles
    (128, 128, 4480, 1),   # 70 steps, split 16, per = 5 steps: slices 14
                           # and 15 are empty and must contribute zeros
    (128, 128, 200, 1),    # K % 64 != 0: stays on the repack kernel
    (128, 136, 4096, 1),   # N % 128 != 0: generic kernel; N % 4 == 0 finish
]


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-8)).item()


def _rn(gen, *s, scale=1.0):
    return (torch.randn(*s, device=DEV, generator=gen) * scale).to(BF)


def _both(fn):
    """fn() with the old kernels (repack TN, scalar finish), then with the
    new ones on every eligible call and each split-K pipeline variant;
    toggles restored."""
    ext = _ext()
    mode, var = ext.get_tn_tr_mode(), ext.get_tn_tr_variant()
    try:
        ext.set_tn_tr(False)
        ext.set_finish_wide(False)
        old = fn()
        ext.set_tn_tr(True)
        ext.set_finish_wide(True)
        new = []
        for v in (1, 2, 3):
            ext.set_tn_tr_variant(v)
            new.append(fn())
        torch.cuda.synchronize()
    finally:
        ext.set_tn_tr_mode(mode)
        ext.set_tn_tr_variant(var)
        ext.set_finish_wide(True)
    return old, new


@functools.lru_cache(maxsize=None)
def _gemm_inputs(M, N, K, G):
    g = torch.Generator(device=DEV).manual_seed(M + 7 * N + 13 * K + G)
    return _rn(g, G, K, M), _rn(g, G, K, N)


@pytest.mark.parametrize("M,N,K,G", GEMM_CASES)
def test_gemm_tn_bitwise_and_fp64(M, N, K, G):
    A, B = _gemm_inputs(M, N, K, G)
    old, new = _both(lambda: _ext().gemm_tn(A, B))
    for v, c in enumerate(new, 1):
        assert torch.equal(old, c), ("variant", v)
    ref = torch.matmul(A.double().transpose(1, 2), B.double())
    r = _rel(new[0], ref)
    print("gemm_tn", (M, N, K, G), "rel", r)
    assert r < TN_BOUND
    # and every element within the any-order f32 accumulation bound
    from _bounds_util import assert_within, gemm_tol
    absprod = torch.matmul(A.double().abs().transpose(1, 2), B.double().abs())
    assert_within(new[0], ref, gemm_tol(ref, absprod, K), "gemm_tn")


def test_finish_wide_alone_bitwise():
    """Old TN kernel under both finish kernels: the re-blocked finish by
    itself (split 16 with two empty slices)."""
    ext = _ext()
    A, B = _gemm_inputs(128, 128, 4480, 1)
    mode = ext.get_tn_tr_mode()
    try:
        ext.set_tn_tr(False)
        ext.set_finish_wide(False)
        a = ext.gemm_tn(A, B)
        ext.set_finish_wide(True)
        b = ext.gemm_tn(A, B)
    finally:
        ext.set_tn_tr_mode(mode)
        ext.set_finish_wide(True)
    assert torch.equal(a, b)


def test_dispatch_lines():
    """K % 64 == 0 calls take gemm_tn_tr (non-split and split-K), K = 200
    stays on the repack kernel, GLOM_TN_TR=0 reverts everything."""
    code = (
        "import torch\n"
        "from glom_pytorch_amd.ops import _load_extension\n"
        "ext = _load_extension()\n"
        "r = lambda *s: torch.randn(*s, device='cuda:0',"
        " dtype=torch.bfloat16)\n"
        "ext.set_tn_tr(%s)\n"
        "for (M, N, K, G) in %r:\n"
        "    ext.gemm_tn(r(G, K, M), r(G, K, N))\n"
        "torch.cuda.synchronize()\n")
    cases = GEMM_CASES[:5]

    def lines(on):
        env = dict(os.environ, GLOM_DISPATCH_DEBUG="1")
        r = subprocess.run([sys.executable, "-c", code % (on, cases)],
                           env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-800:]
        out = [ln for ln in r.stderr.splitlines() if "[dispatch] L2" in ln]
        assert len(out) == len(cases), out
        return out

    on = lines(True)
    for (M, N, K, G), ln in zip(cases, on):
        assert "M%d N%d K%d " % (M, N, K) in ln, ln
        want_sk = 16 if K >= 4096 else 1
        assert "sk=%d " % want_sk in ln, ln
        assert ("tn_tr=1" if K % 64 == 0 else "tn_tr=0") in ln, ln
    assert all("tn_tr=0" in ln for ln in lines(False))


def test_ff_bwd_dw_table_strided_bitwise():
    """Bottom-up dW: the B operand of dW1 is table-resolved (tokens, then
    levels[..., g-1, :] with row stride L*d), dW2's A operand dY[..., g, :]
    has row stride G*d: the alignment / stride case of the DMA copy.
    Both are split-K (K = 4096, 8 tiles -> split 16)."""
    Bt, N, L, d, m4 = 16, 256, 2, 128, 512
    G, M = L, Bt * N
    g = torch.Generator(device=DEV).manual_seed(99)
    dY = _rn(g, Bt, N, G, d)
    dH = _rn(g, G, M, m4)
    Hact = _rn(g, G, M, m4)
    tokens = _rn(g, Bt, N, d)
    levels = _rn(g, Bt, N, L, d)
    old, new = _both(lambda: _ext().ff_bwd_dw(dY, dH, tokens, levels, None,
                                              Hact, 0))
    for res in new:
        for o, n in zip(old, res):
            assert o.numel() > 0 and torch.equal(o, n)
    dW1, dW2, _ = new[0]
    xs = [tokens.double().reshape(M, d)] + [
        levels.double()[..., k, :].reshape(M, d) for k in range(L - 1)]
    for k in range(G):
        r1 = dH[k].double().t() @ xs[k]
        r2 = dY.double()[..., k, :].reshape(M, d).t() @ Hact[k].double()
        e1 = _rel(dW1[k * m4:(k + 1) * m4], r1)
        e2 = _rel(dW2[k * d:(k + 1) * d], r2)
        print("ff_bwd_dw group", k, "rel", e1, e2)
        assert e1 < TN_BOUND and e2 < TN_BOUND


def test_consensus_bwd_bitwise():
    """Smallest fused consensus backward (N = 256): dv and dk-hat are
    K = 256 non-split TN products over sout-strided operands; they reach
    the caller through dLevels = knorm_combine(dk-hat, dv, dq), whose other
    inputs do not depend on the toggle."""
    import math
    import torch.nn.functional as F
    Bt, N, L, d = 2, 256, 2, 128
    g = torch.Generator(device=DEV).manual_seed(5)
    lv = _rn(g, Bt, N, L, d)
    dOut = _rn(g, Bt, N, L, d)
    ext = _ext()
    _, probs, rnorm = ext.consensus_fwd(lv, False, None)
    old, new = _both(lambda: ext.consensus_bwd(dOut, lv, probs, rnorm,
                                               False, None))
    for res in new:
        assert torch.equal(old, res)
    x = lv.double().requires_grad_()
    sim = torch.einsum("bild,bjld->blij", x,
                       F.normalize(x, dim=-1)) / math.sqrt(d)
    eye = torch.eye(N, device=DEV, dtype=torch.bool)
    sim = sim.masked_fill(eye.view(1, 1, N, N), -5e-4)
    ref = torch.einsum("blij,bjld->bild", sim.softmax(-1), x)
    (dref,) = torch.autograd.grad(ref, x, dOut.double())
    r = _rel(new[0], dref)
    print("consensus_bwd rel", r)
    assert r < TN_BOUND


def test_patch_embed_dw_finish_bitwise():
    """Patch-embed dW: (dout x Kp) with Kp = 640 padded columns, split-K
    finish into the padded buffer, then k_slice_cols to 588 columns."""
    Bt, P, dout = 16, 14, 128
    g = torch.Generator(device=DEV).manual_seed(11)
    img = _rn(g, Bt, 3, 224, 224)
    w = _rn(g, dout, P * P * 3, scale=0.04)
    b = _rn(g, dout)
    ext = _ext()
    tokens, X = ext.patch_embed_fwd(img, w, b, P)
    assert X.shape[-1] == 640
    dTok = _rn(g, *tokens.shape)
    old, new = _both(lambda: ext.patch_embed_bwd(dTok, X, w, P, 224, 224,
                                                 False)[0])
    for res in new:
        assert torch.equal(old, res)
    M = Bt * 256
    ref = dTok.double().reshape(M, dout).t() @ X.double().reshape(M, 640)
    r = _rel(new[0], ref[:, :P * P * 3])
    print("patch_embed dW rel", r)
    assert r < TN_BOUND
