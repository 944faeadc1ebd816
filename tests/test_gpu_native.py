"""GPU parity tests: the CDNA4 HIP engine vs plain-PyTorch fp32 references.

Every op test compares the bf16 HIP kernel against fp32 torch math computed
from the SAME bf16 inputs, so tolerances only cover bf16 rounding inside the
kernels.
"""

import os

import pytest
import torch

from glom_pytorch_amd import Glom

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

CFG = dict(dim=64, levels=3, image_size=32, patch_size=8)
DEV = "cuda:0"


def _rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _models(**kw):
    cfg = {**CFG, **kw}
    torch.manual_seed(0)
    m32 = Glom(**cfg).to(DEV)
    m32.force_eager = True
    mbf = Glom(**cfg).to(DEV)
    mbf.load_state_dict(m32.state_dict())
    mbf = mbf.to(torch.bfloat16)
    return m32, mbf


def test_extension_is_in_tree():
    from glom_pytorch_amd.ops import _load_extension
    ext = _load_extension()
    import glom_pytorch_amd
    pkg = os.path.dirname(os.path.dirname(glom_pytorch_amd.__file__))
    assert ext.__file__.startswith(pkg), ext.__file__


@pytest.mark.parametrize("kw", [
    {},
    dict(consensus_self=True),
    dict(local_consensus_radius=2),
])
def test_forward_parity(kw):
    m32, mbf = _models(**kw)
    img = torch.randn(2, 3, 32, 32, device=DEV)
    ref = m32(img, iters=3)
    out = mbf(img.to(torch.bfloat16), iters=3)
    assert out.dtype == torch.bfloat16
    err = _rel_err(out, ref)
    assert err < 2e-2, err


def test_forward_parity_return_all_and_state():
    m32, mbf = _models()
    img = torch.randn(2, 3, 32, 32, device=DEV)
    ref = m32(img, iters=4, return_all=True)
    out = mbf(img.to(torch.bfloat16), iters=4, return_all=True)
    assert out.shape == ref.shape
    assert _rel_err(out, ref) < 2e-2
    # stateful continuation
    ref2 = m32(img, iters=2, levels=ref[-1])
    out2 = mbf(img.to(torch.bfloat16), iters=2, levels=out[-1])
    assert _rel_err(out2, ref2) < 3e-2


def test_forward_parity_ragged_patches():
    # N=9 patches (3x3 grid): exercises GEMM M/N/K tails and softmax tails
    m32, mbf = _models(image_size=24, patch_size=8)
    img = torch.randn(2, 3, 24, 24, device=DEV)
    ref = m32(img, iters=3)
    out = mbf(img.to(torch.bfloat16), iters=3)
    assert _rel_err(out, ref) < 2e-2


def test_backward_parity():
    m32, mbf = _models()
    img = torch.randn(2, 3, 32, 32, device=DEV)
    for model, x in ((m32, img), (mbf, img.to(torch.bfloat16))):
        out = model(x, iters=3, return_all=True)
        # touch ALL levels at the end plus the top level mid-trajectory so
        # every parameter (incl. the patch embedding) receives gradient
        loss = (out[-1].float().pow(2).mean()
                + out[2, :, :, -1].float().pow(2).mean())
        model.zero_grad()
        loss.backward()
    for (n32, p32), (nbf, pbf) in zip(m32.named_parameters(),
                                      mbf.named_parameters()):
        assert n32 == nbf
        g32, gbf = p32.grad.float(), pbf.grad.float()
        assert g32.norm() > 0, (n32, "fp32 grad unexpectedly zero")
        cos = torch.nn.functional.cosine_similarity(
            g32.flatten(), gbf.flatten(), dim=0).item()
        assert cos > 0.99, (n32, cos)
        rel = _rel_err(gbf, g32)
        assert rel < 0.15, (n32, rel)


def test_grouped_ff_op():
    from glom_pytorch_amd.ops.functional import GroupedFFFn
    torch.manual_seed(1)
    B, N, L, d = 2, 16, 3, 64
    m4 = 4 * d
    bf = torch.bfloat16
    tokens = torch.randn(B, N, d, device=DEV, dtype=bf)
    levels = torch.randn(B, N, L, d, device=DEV, dtype=bf)
    pos = torch.randn(N, d, device=DEV, dtype=bf)
    w1 = torch.randn(L * m4, d, device=DEV, dtype=bf) * 0.05
    b1 = torch.randn(L * m4, device=DEV, dtype=bf)
    w2 = torch.randn(L * d, m4, device=DEV, dtype=bf) * 0.05
    b2 = torch.randn(L * d, device=DEV, dtype=bf)

    out = GroupedFFFn.apply(tokens, levels, None, w1, b1, w2, b2, 0)
    # fp32 reference from the same bf16 inputs
    xs = [tokens.float()] + [levels[..., g, :].float() for g in range(L - 1)]
    for g in range(L):
        h = xs[g] @ w1.float()[g * m4:(g + 1) * m4].t() + b1.float()[g * m4:(g + 1) * m4]
        y = torch.nn.functional.gelu(h) @ w2.float()[g * d:(g + 1) * d].t() \
            + b2.float()[g * d:(g + 1) * d]
        err = _rel_err(out[..., g, :], y)
        assert err < 1e-2, (g, err)

    # top-down mode with fused pos add (groups L-1)
    w1t, b1t = w1[:(L - 1) * m4], b1[:(L - 1) * m4]
    w2t, b2t = w2[:(L - 1) * d], b2[:(L - 1) * d]
    out_td = GroupedFFFn.apply(None, levels, pos, w1t, b1t, w2t, b2t, 1)
    for g in range(L - 1):
        x = (levels[..., g + 1, :] + pos.view(1, N, d)).float()
        h = x @ w1t.float()[g * m4:(g + 1) * m4].t() + b1t.float()[g * m4:(g + 1) * m4]
        y = torch.nn.functional.gelu(h) @ w2t.float()[g * d:(g + 1) * d].t() \
            + b2t.float()[g * d:(g + 1) * d]
        err = _rel_err(out_td[..., g, :], y)
        assert err < 1e-2, (g, err)

    # per element, stage by stage: each GEMM against fp64 of the bf16
    # operands the kernel itself read (x and the returned Hact)
    from _bounds_util import assert_within, gemm_tol
    from glom_pytorch_amd.ops import _load_extension
    ext = _load_extension()
    M = B * N
    td_x = [(levels[..., g + 1, :] + pos.view(1, N, d)) for g in range(L - 1)]
    for mode, args, xin, res in (
            (0, (tokens, levels, None, w1, b1, w2, b2),
             [tokens] + [levels[..., g, :] for g in range(L - 1)], out),
            (1, (None, levels, pos, w1t, b1t, w2t, b2t), td_x, out_td)):
        Y, Hpre, Hact, _ = ext.grouped_ff_fwd(*args, mode)
        assert torch.equal(Y, res)
        W1, B1, W2, B2 = (t.double() for t in args[3:])
        for g in range(len(xin)):
            x = xin[g].double().reshape(M, d)
            wa, ba = W1[g * m4:(g + 1) * m4], B1[g * m4:(g + 1) * m4]
            h = x @ wa.t() + ba
            assert_within(Hpre[g], h, gemm_tol(
                h, x.abs() @ wa.abs().t() + ba.abs(), d), "Hpre")
            a = Hact[g].double()
            wb, bb = W2[g * d:(g + 1) * d], B2[g * d:(g + 1) * d]
            y = a @ wb.t() + bb
            assert_within(Y[..., g, :].reshape(M, d), y, gemm_tol(
                y, a.abs() @ wb.abs().t() + bb.abs(), m4), "Y")


def test_consensus_op():
    from glom_pytorch_amd.ops.functional import ConsensusFn
    import math
    import torch.nn.functional as F
    torch.manual_seed(2)
    B, N, L, d = 2, 16, 3, 64
    levels = torch.randn(B, N, L, d, device=DEV, dtype=torch.bfloat16)
    for attend_self in (True, False):
        out = ConsensusFn.apply(levels, attend_self, None)
        lv = levels.float()
        q, k = lv, F.normalize(lv, dim=-1)
        sim = torch.einsum("bild,bjld->blij", q, k) / math.sqrt(d)
        if not attend_self:
            eye = torch.eye(N, device=DEV, dtype=torch.bool)
            sim = sim.masked_fill(eye.view(1, 1, N, N), -5e-4)
        ref = torch.einsum("blij,bjld->bild", sim.softmax(-1), lv)
        err = _rel_err(out, ref)
        assert err < 1e-2, (attend_self, err)
        # per element: the AV product against fp64 of the stored probs
        from _bounds_util import assert_within, gemm_tol
        from glom_pytorch_amd.ops import _load_extension
        out2, probs, _ = _load_extension().consensus_fwd(levels, attend_self,
                                                         None)
        assert torch.equal(out2, out)
        P, x = probs.double(), levels.double().permute(0, 2, 1, 3)
        o64 = torch.matmul(P, x).permute(0, 2, 1, 3)
        oabs = torch.matmul(P, x.abs()).permute(0, 2, 1, 3)
        assert_within(out, o64, gemm_tol(o64, oabs, N), "out")


def test_consensus_op_backward():
    from glom_pytorch_amd.ops.functional import ConsensusFn
    import math
    import torch.nn.functional as F
    torch.manual_seed(3)
    B, N, L, d = 2, 16, 2, 64
    lv_bf = torch.randn(B, N, L, d, device=DEV, dtype=torch.bfloat16,
                        requires_grad=True)
    out = ConsensusFn.apply(lv_bf, False, None)
    g = torch.randn_like(out)
    (dlev,) = torch.autograd.grad(out, lv_bf, g)

    lv = lv_bf.detach().float().requires_grad_(True)
    q, k = lv, F.normalize(lv, dim=-1)
    sim = torch.einsum("bild,bjld->blij", q, k) / math.sqrt(d)
    eye = torch.eye(N, device=DEV, dtype=torch.bool)
    sim = sim.masked_fill(eye.view(1, 1, N, N), -5e-4)
    ref = torch.einsum("blij,bjld->bild", sim.softmax(-1), lv)
    (dref,) = torch.autograd.grad(ref, lv, g.float())
    err = _rel_err(dlev, dref)
    assert err < 3e-2, err


def test_flagship_shapes_native():
    torch.manual_seed(0)
    m = Glom(dim=512, levels=6, image_size=224, patch_size=14)
    m = m.to(DEV, torch.bfloat16)
    img = torch.randn(2, 3, 224, 224, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        out = m(img, iters=12, return_all=True)
    assert out.shape == (13, 2, 256, 6, 512)
    assert torch.isfinite(out.float()).all()


def test_parity_fast_tile_shapes():
    """Shapes that are full 128-multiples exercise the tuned glds NT and
    repack TN kernels (small-dim tests above cover the generic fallback)."""
    cfg = dict(dim=128, levels=3, image_size=128, patch_size=8)  # N=256
    torch.manual_seed(0)
    m32 = Glom(**cfg).to(DEV)
    m32.force_eager = True
    mbf = Glom(**cfg).to(DEV)
    mbf.load_state_dict(m32.state_dict())
    mbf = mbf.to(torch.bfloat16)
    img = torch.randn(1, 3, 128, 128, device=DEV)
    for model, x in ((m32, img), (mbf, img.to(torch.bfloat16))):
        out = model(x, iters=3, return_all=True)
        loss = out[-1].float().pow(2).mean()
        model.zero_grad()
        loss.backward()
    out32 = m32(img, iters=3)
    outbf = mbf(img.to(torch.bfloat16), iters=3)
    assert _rel_err(outbf, out32) < 2e-2
    for (n32, p32), (nbf, pbf) in zip(m32.named_parameters(),
                                      mbf.named_parameters()):
        g32, gbf = p32.grad.float(), pbf.grad.float()
        cos = torch.nn.functional.cosine_similarity(
            g32.flatten(), gbf.flatten(), dim=0).item()
        assert cos > 0.99, (n32, cos)


@pytest.mark.parametrize("attend_self,radius", [(False, 0), (True, 0),
                                                (False, 3)])
def test_consensus_fused_softmax_n256(attend_self, radius):
    """N=256 rides the fused scores+softmax / dP+softmax-bwd epilogues;
    verify against fp32 einsum math including the masked variants."""
    import math
    import torch.nn.functional as F
    from glom_pytorch_amd.ops.functional import ConsensusFn
    torch.manual_seed(5)
    B, N, L, d = 1, 256, 2, 64
    lv = torch.randn(B, N, L, d, device=DEV, dtype=torch.bfloat16,
                     requires_grad=True)
    mask = None
    if radius:
        side = 16
        hh, ww = torch.meshgrid(torch.arange(side), torch.arange(side),
                                indexing="ij")
        coords = torch.stack((hh, ww)).float().view(2, -1).t()
        mask = (torch.cdist(coords, coords) > radius).view(1, N, N).to(DEV)
    out = ConsensusFn.apply(lv, attend_self, mask)
    g = torch.randn_like(out)
    (dlev,) = torch.autograd.grad(out, lv, g)

    x = lv.detach().float().requires_grad_(True)
    sim = torch.einsum("bild,bjld->blij", x,
                       F.normalize(x, dim=-1)) / math.sqrt(d)
    if not attend_self:
        eye = torch.eye(N, device=DEV, dtype=torch.bool)
        sim = sim.masked_fill(eye.view(1, 1, N, N), -5e-4)
    if mask is not None:
        sim = sim.masked_fill(mask.view(1, 1, N, N), -3.3895e38)
    ref = torch.einsum("blij,bjld->bild", sim.softmax(-1), x)
    (dref,) = torch.autograd.grad(ref, x, g.float())
    assert _rel_err(out, ref) < 1e-2
    assert _rel_err(dlev, dref) < 3e-2


def test_forward_determinism_race_smoke():
    """Two identical forwards must agree bitwise: the forward path has no
    atomics or cross-block races by construction (SURVEY.md §5 race
    detection strategy)."""
    torch.manual_seed(0)
    m = Glom(dim=512, levels=6, image_size=224, patch_size=14)
    m = m.to(DEV, torch.bfloat16)
    img = torch.randn(2, 3, 224, 224, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        a = m(img, iters=4)
        b = m(img, iters=4)
    assert torch.equal(a, b)


def test_denoising_trainer_gpu_step():
    from glom_pytorch_amd.parallel.trainer import DenoisingTrainer
    torch.manual_seed(0)
    m = Glom(**CFG).to(DEV, torch.bfloat16)
    tr = DenoisingTrainer(m, noise_std=0.5, decode_step=2)
    img = torch.randn(2, 3, 32, 32, device=DEV, dtype=torch.bfloat16)
    l1 = tr.step(img, iters=3)
    l2 = tr.step(img, iters=3)
    assert l1 > 0 and l2 > 0
    for n, p in m.named_parameters():
        assert torch.isfinite(p.float()).all(), n


def test_levels2_minimum_native():
    """levels=2: top_down has a single group (G=1) — smallest table case."""
    torch.manual_seed(0)
    m32 = Glom(dim=64, levels=2, image_size=32, patch_size=8).to(DEV)
    m32.force_eager = True
    mbf = Glom(dim=64, levels=2, image_size=32, patch_size=8).to(DEV)
    mbf.load_state_dict(m32.state_dict())
    mbf = mbf.to(torch.bfloat16)
    img = torch.randn(2, 3, 32, 32, device=DEV)
    ref = m32(img, iters=3)
    out = mbf(img.to(torch.bfloat16), iters=3)
    assert _rel_err(out, ref) < 2e-2


def test_batch1_native():
    torch.manual_seed(0)
    m = Glom(dim=512, levels=6, image_size=224, patch_size=14)
    m = m.to(DEV, torch.bfloat16)
    img = torch.randn(1, 3, 224, 224, device=DEV, dtype=torch.bfloat16)
    out = m(img, iters=12)
    assert out.shape == (1, 256, 6, 512)
    assert torch.isfinite(out.float()).all()


def test_backward_singlestream_path_matches():
    """The opt-out single-stream mega-backward must agree with the default
    stream-forked backward."""
    import os
    torch.manual_seed(0)
    m = Glom(**CFG).to(DEV, torch.bfloat16)
    img = torch.randn(2, 3, 32, 32, device=DEV, dtype=torch.bfloat16)

    def grads():
        m.zero_grad()
        out = m(img, iters=3, return_all=True)
        out[-1].float().pow(2).mean().backward()
        return {n: p.grad.clone() for n, p in m.named_parameters()}

    g_fork = grads()
    os.environ["GLOM_NO_BWD_STREAMS"] = "1"
    try:
        g_single = grads()
    finally:
        del os.environ["GLOM_NO_BWD_STREAMS"]
    # every reduction, the dB1 column sum included, runs in fixed order
    for n in g_fork:
        assert torch.equal(g_fork[n], g_single[n]), n


def test_trainer_checkpoint_resume_gpu():
    """Checkpoint/resume on GPU: identical weights and RNG-driven noise
    give identical continuation losses."""
    from glom_pytorch_amd.parallel.trainer import DenoisingTrainer
    import tempfile, os
    torch.manual_seed(0)
    m = Glom(**CFG).to(DEV, torch.bfloat16)
    tr = DenoisingTrainer(m, noise_std=0.5, decode_step=2)
    img = torch.randn(2, 3, 32, 32, device=DEV, dtype=torch.bfloat16)
    tr.step(img, iters=3)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ck.pt")
        tr.save_checkpoint(path)
        m2 = Glom(**CFG).to(DEV, torch.bfloat16)
        tr2 = DenoisingTrainer(m2, noise_std=0.5, decode_step=2)
        tr2.load_checkpoint(path)
        la = tr.step(img, iters=3)
        lb = tr2.step(img, iters=3)
    assert tr2.step_idx == 2
    assert abs(la - lb) < 1e-4, (la, lb)
