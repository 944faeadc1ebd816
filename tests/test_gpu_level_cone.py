"""Level cone: backward ops restricted to the live groups / levels.

When the loss reads the trajectory at one time and at levels >=
``loss_level_min`` only, the gradient arriving at iteration t is exactly
zero below ``lo_t``; the backward skips those groups and fills in zeros.
A GEMM of zeros gives zeros, so every result must equal (``torch.equal``,
which takes -0 == +0) what the same build computes with the hint off: the
full call on the same, partly zero, incoming gradient.

Op-level shapes: B=2 N=256 L=4 d=256 (m4=1024), every first live group.
Dispatch pinning (d=512 L=6 N=256, m4=2048), the smallest shapes at which a
``run_gemm`` gate would flip between all groups and one group:
  B=16: dW1 / dW2 have K = B*N = 4096 and 64 tiles per group; all G groups
        give split-K 5 (bottom-up, 384 tiles) where one alone would get 16
  B=32: the top-down dX grid is 2*32*5 = 320 nt8p blocks, 64 for one group
        (below the kernel's 256-block gate)
"""

import copy
import functools

import pytest
import torch

from glom_pytorch_amd import Glom

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"
BF = torch.bfloat16
OUT6 = ("dTokens", "dLevels", "dW1", "dB1", "dW2", "dB2")


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


@functools.lru_cache(maxsize=None)
def _ff_case(B, N, L, d, mode):
    """Inputs, the forward's saved tensors and a random dY of one grouped
    FF call; built once per shape and left unchanged."""
    ext = _ext()
    G = L if mode == 0 else L - 1
    m4 = 4 * d
    g = torch.Generator(device=DEV).manual_seed(77 + mode + B)

    def rn(*s, scale=1.0):
        return (torch.randn(*s, device=DEV, generator=g) * scale).to(BF)
    c = dict(tokens=rn(B, N, d) if mode == 0 else None,
             levels=rn(B, N, L, d), pos=rn(N, d) if mode == 1 else None,
             w1=rn(G * m4, d, scale=0.04), b1=rn(G * m4),
             w2=rn(G * d, m4, scale=0.04), b2=rn(G * d),
             dY=rn(B, N, G, d), G=G, m4=m4)
    _, c["Hpre"], c["Hact"], c["td_in"] = ext.grouped_ff_fwd(
        c["tokens"], c["levels"], c["pos"], c["w1"], c["b1"], c["w2"],
        c["b2"], mode)
    c["w1t"] = c["w1"].view(G, m4, d).transpose(1, 2).contiguous()
    c["w2t"] = c["w2"].view(G, d, m4).transpose(1, 2).contiguous()
    return c


def _dy(c, g_lo):
    dY = c["dY"].clone()
    dY[:, :, :g_lo] = 0
    return dY


def _ff_bwd(c, mode, dY, g_lo):
    return _ext().grouped_ff_bwd(
        dY, c["tokens"], c["levels"], c["pos"], c["w1"], c["w2"], c["Hpre"],
        c["Hact"], mode, c["w1t"], c["w2t"], c["td_in"], g_lo)


def _assert_six(got, ref, what):
    for name, a, b in zip(OUT6, got, ref):
        assert a.shape == b.shape, (what, name)
        assert torch.equal(a, b), (what, name)


# ------------------------------ 1. op level --------------------------- #

@pytest.mark.parametrize("mode", [0, 1])
def test_grouped_ff_bwd_every_g_lo(mode):
    c = _ff_case(2, 256, 4, 256, mode)
    for g_lo in range(c["G"] + 1):
        dY = _dy(c, g_lo)
        _assert_six(_ff_bwd(c, mode, dY, g_lo), _ff_bwd(c, mode, dY, 0),
                    f"mode {mode} g_lo {g_lo}")


@pytest.mark.parametrize("mode", [0, 1])
def test_ff_bwd_trio_every_g_lo(mode):
    ext = _ext()
    B, N, L, d = 2, 256, 4, 256
    c = _ff_case(B, N, L, d, mode)

    def trio(dY, g_lo):
        dh, db1 = ext.ff_bwd_dh(dY, c["w2t"], c["Hpre"], g_lo)
        dt, dl = ext.ff_bwd_dx(dh, c["w1t"], c["tokens"], B, N, L, mode,
                               g_lo)
        w1, w2, b2 = ext.ff_bwd_dw(dY, dh, c["tokens"], c["levels"],
                                   c["pos"], c["Hact"], mode, c["td_in"],
                                   g_lo)
        return dh, (dt, dl, w1, db1, w2, b2)

    for g_lo in range(c["G"] + 1):
        dY = _dy(c, g_lo)
        dh, six = trio(dY, g_lo)
        dh0, six0 = trio(dY, 0)
        _assert_six(six, six0, f"trio mode {mode} g_lo {g_lo}")
        # dead groups of dHpre are neither written nor read
        assert torch.equal(dh[g_lo:], dh0[g_lo:])
        # and the trio agrees with the one-call op
        _assert_six(six, _ff_bwd(c, mode, dY, 0), "trio vs grouped")


def test_consensus_bwd_every_l_lo():
    ext = _ext()
    B, N, L, d = 2, 256, 4, 256
    g = torch.Generator(device=DEV).manual_seed(5)
    levels = torch.randn(B, N, L, d, device=DEV, generator=g).to(BF)
    dOut0 = torch.randn(B, N, L, d, device=DEV, generator=g).to(BF)
    for attend_self in (False, True):
        _, probs, rnorm = ext.consensus_fwd(levels, attend_self, None)
        for l_lo in range(L + 1):
            dOut = dOut0.clone()
            dOut[:, :, :l_lo] = 0
            got = ext.consensus_bwd(dOut, levels, probs, rnorm, attend_self,
                                    None, l_lo)
            ref = ext.consensus_bwd(dOut, levels, probs, rnorm, attend_self,
                                    None, 0)
            assert torch.equal(got, ref), (attend_self, l_lo)
            assert not got[:, :, :l_lo].any()


def test_consensus_bwd_unfused_path_every_l_lo():
    """N != 256 takes the GEMM + row-softmax-backward path."""
    ext = _ext()
    B, N, L, d = 3, 64, 3, 64
    g = torch.Generator(device=DEV).manual_seed(6)
    levels = torch.randn(B, N, L, d, device=DEV, generator=g).to(BF)
    dOut0 = torch.randn(B, N, L, d, device=DEV, generator=g).to(BF)
    _, probs, rnorm = ext.consensus_fwd(levels, False, None)
    for l_lo in range(L + 1):
        dOut = dOut0.clone()
        dOut[:, :, :l_lo] = 0
        got = ext.consensus_bwd(dOut, levels, probs, rnorm, False, None,
                                l_lo)
        ref = ext.consensus_bwd(dOut, levels, probs, rnorm, False, None, 0)
        assert torch.equal(got, ref), l_lo


# -------------------------- 2. dispatch pinning ----------------------- #

@pytest.mark.parametrize("B", [16, 32], ids=["splitk_gate", "nt8p_gate"])
@pytest.mark.parametrize("mode", [0, 1])
def test_one_live_group_keeps_the_full_calls_kernels(B, mode):
    """Outputs only: a different kernel or split-K factor for the one live
    group would change its f32 summation order and with it the bits."""
    c = _ff_case(B, 256, 6, 512, mode)
    g_lo = c["G"] - 1
    dY = _dy(c, g_lo)
    got = _ff_bwd(c, mode, dY, g_lo)
    ref = _ff_bwd(c, mode, dY, 0)
    _assert_six(got, ref, f"B {B} mode {mode}")
    assert got[2][g_lo * c["m4"]:].float().abs().sum() > 0   # live dW1


# ------------------------------ 3. model ------------------------------ #

MODEL = dict(dim=256, levels=4, image_size=112, patch_size=7)
PATHS = {"fork3": {}, "fork4": {"GLOM_BWD_FORK": "4"},
         "single_stream": {"GLOM_NO_BWD_STREAMS": "1"}}


@functools.lru_cache(maxsize=None)
def _model_and_img():
    torch.manual_seed(0)
    m = Glom(**MODEL).to(DEV, BF)
    img = torch.randn(2, 3, 112, 112, device=DEV).to(BF)
    return m, img


@pytest.fixture
def check_mode():
    from glom_pytorch_amd import ops
    ops.set_check_level_cone(True)
    yield
    ops.set_check_level_cone(False)


def _grads(grad_iters, loss_levels, loss_level_min):
    m, img = _model_and_img()
    m.zero_grad(set_to_none=True)
    traj = m(img, iters=6, return_all=True, grad_iters=grad_iters,
             loss_level_min=loss_level_min)
    traj[grad_iters][:, :, loss_levels].float().pow(2).sum().backward()
    torch.cuda.synchronize()
    return {n: p.grad.clone() for n, p in m.named_parameters()
            if p.grad is not None}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("grad_iters,lmin,loss_levels", [
    (5, 3, slice(3, 4)),     # lo_t = 3, 2, 1, 0, 0
    (3, 3, slice(3, 4)),     # lo_t = 3, 2, 1: bottom-up group 0 never live
    (5, 1, slice(1, 4)),     # loss on levels 1..3
])
def test_model_gradients_equal_with_and_without_the_hint(
        path, grad_iters, lmin, loss_levels, monkeypatch, check_mode):
    for k in ("GLOM_BWD_FORK", "GLOM_NO_BWD_STREAMS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    ref = _grads(grad_iters, loss_levels, None)
    got = _grads(grad_iters, loss_levels, lmin)
    assert set(got) == set(ref) and len(ref) >= 10
    for n in ref:
        assert torch.equal(got[n], ref[n]), n
    if grad_iters == 3 and lmin == 3:
        for n in ref:
            if n.startswith("image_to_tokens"):
                assert not ref[n].any() and not got[n].any(), n
    assert ref["bottom_up.net.1.weight"].float().abs().sum() > 0


# --------------------------- 4. wrong promise -------------------------- #

def test_check_mode_catches_a_broken_promise(check_mode):
    """Host-side comparison of a gradient slice with zero; nothing faults."""
    with pytest.raises(RuntimeError, match=r"iteration 4 .* level 0"):
        _grads(5, slice(0, 1), 3)


def test_check_mode_is_off_by_default_and_refuses_capture():
    from glom_pytorch_amd.ops import functional as Fn
    assert Fn.CHECK_LEVEL_CONE is False
    dnew = torch.zeros(2, 8, 4, 16, device=DEV, dtype=BF)
    Fn._check_cone(dnew, 3, 0)            # all zero below level 3: passes
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="stream capture"):
        with torch.cuda.graph(g):
            dnew2 = dnew + 1              # something to capture
            Fn._check_cone(dnew2, 3, 0)   # refuses before any host sync
    torch.cuda.synchronize()


# ------------------------------ 5. trainer ---------------------------- #

def _train(level_cone, graph_step, **kw):
    from glom_pytorch_amd.parallel.trainer import DenoisingTrainer
    torch.manual_seed(0)
    m = Glom(**MODEL).to(DEV, BF)
    tr = DenoisingTrainer(m, lr=1e-3, decode_step=4, graph_step=graph_step,
                          level_cone=level_cone, **kw)
    assert tr.level_cone is level_cone
    img = torch.randn(2, 3, 112, 112, device=DEV).to(BF)
    torch.manual_seed(1)
    losses = [tr.step(img, iters=6) for _ in range(3)]
    torch.cuda.synchronize()
    return (losses, [q.detach().clone() for q in tr._params],
            [w.clone() for w in tr.master])


@pytest.mark.parametrize("kw", [
    dict(graph_step=True), dict(graph_step=False),
    dict(graph_step=False, contrast_weight=0.1),
    dict(graph_step=True, contrast_weight=0.1, contrast_level=1),
], ids=["captured", "eager_launch", "contrast", "contrast_level1_captured"])
def test_trainer_steps_equal_with_and_without_the_cone(kw, monkeypatch):
    monkeypatch.delenv("GLOM_NO_LEVEL_CONE", raising=False)
    l1, p1, w1 = _train(True, **kw)
    l0, p0, w0 = _train(False, **kw)
    assert l1 == l0 and all(x == x for x in l1)
    for a, b in zip(p1 + w1, p0 + w0):
        assert torch.equal(a, b)


def test_env_opt_out(monkeypatch):
    from glom_pytorch_amd.parallel.trainer import DenoisingTrainer
    monkeypatch.setenv("GLOM_NO_LEVEL_CONE", "1")
    m = copy.deepcopy(_model_and_img()[0])
    tr = DenoisingTrainer(m, graph_step=False)
    assert tr.level_cone is False and tr._loss_level_min() is None
