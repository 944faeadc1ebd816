"""Level-mix fusion: the mix of iteration t also writes iteration t+1's
top-down input (levels[..., 1:, :] + pos) and row norms, from the rounded
values it stores, so k_add_pos and k_rnorm are not launched again.

Both must be bit-identical to the standalone kernels on the same mixed
tensor. The mix emits them at d = 512 only (one wave = one row, k_rnorm's
summation order); every other d must fall back: empty extras, standalone
kernels in the consumers. Standalone references come from the ops that own
the kernels: ``grouped_ff_fwd`` mode 1 returns its td_in, ``consensus_fwd``
its rnorm. Every comparison is ``torch.equal`` within one build.
"""

import functools

import pytest
import torch

import _loop_invariant_util as U
from _loop_invariant_util import BF, DEV, MODEL256, MODEL512

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

SWITCH = "set_mix_fusion"
CFGS = {"dim512": MODEL512, "dim256_fallback": MODEL256}


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


@functools.lru_cache(maxsize=None)
def _case(B, N, L, d):
    g = torch.Generator(device=DEV).manual_seed(31 + N + L + d)
    G, m4 = L - 1, 4 * d

    def rn(*s, scale=1.0):
        return (torch.randn(*s, device=DEV, generator=g) * scale).to(BF)
    return dict(levels=rn(B, N, L, d), bu=rn(B, N, L, d), cons=rn(B, N, L, d),
                td=rn(B, N, G, d), pos=rn(N, d),
                w1=rn(G * m4, d, scale=0.04), b1=rn(G * m4),
                w2=rn(G * d, m4, scale=0.04), b2=rn(G * d))


def _top_down(c, mixed, td_in=None):
    return _ext().grouped_ff_fwd(None, mixed, c["pos"], c["w1"], c["b1"],
                                 c["w2"], c["b2"], 1, True, False, td_in)


# ------------------------------ op level ------------------------------ #

@pytest.mark.parametrize("N", [64, 9], ids=["N64", "N9_ragged"])
@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("d", [64, 256, 512, 1024])
def test_extras_equal_the_standalone_kernels(d, L, N):
    ext = _ext()
    B = 3
    c = _case(B, N, L, d)
    ref = ext.level_mix_fwd(c["levels"], c["bu"], c["td"], c["cons"])
    out, td_next, rn_next = ext.level_mix_fwd_next(
        c["levels"], c["bu"], c["td"], c["cons"], None, 0, None, c["pos"])
    assert torch.equal(out, ref)
    # the standalone kernels on the same mixed tensor
    tdY, _, _, td_in = _top_down(c, out)
    cons, probs, rnorm = ext.consensus_fwd(out, True, None)
    assert td_in.shape == (B, N, L - 1, d) and rnorm.shape == (B, L, N)
    if d != 512:
        # excluded shape: nothing emitted, the consumers run their kernels
        assert td_next.numel() == 0 and rn_next.numel() == 0
        return
    assert td_next.shape == td_in.shape and rn_next.shape == rnorm.shape
    assert rn_next.dtype == torch.float32
    assert torch.equal(td_next, td_in)
    assert torch.equal(rn_next, rnorm)
    # consumers given the ready tensors: same results, no copy
    tdY2, _, _, td_in2 = _top_down(c, out, td_next)
    assert td_in2.data_ptr() == td_next.data_ptr()
    assert torch.equal(tdY2, tdY)
    cons2, probs2, rnorm2 = ext.consensus_fwd(out, True, None, rn_next)
    assert rnorm2.data_ptr() == rn_next.data_ptr()
    assert torch.equal(cons2, cons) and torch.equal(probs2, probs)


def test_extras_with_kept_level0_and_slab():
    """Both loop invariants in one launch, written into a trajectory slab."""
    ext = _ext()
    B, N, L, d = 2, 64, 4, 512
    c = _case(B, N, L, d)
    ref, td_ref, rn_ref = ext.level_mix_fwd_next(
        c["levels"], c["bu"], c["td"], c["cons"], None, 0, None, c["pos"])
    later = c["bu"].clone()
    later[:, :, 0] = float("nan")
    slab = torch.zeros(2, B, N, L, d, device=DEV, dtype=BF)
    out, td_next, rn_next = ext.level_mix_fwd_next(
        c["levels"], later, c["td"], c["cons"], slab, 1, c["bu"][:, :, 0, :],
        c["pos"])
    assert torch.equal(out, ref) and torch.equal(slab[1], ref)
    assert torch.equal(td_next, td_ref) and torch.equal(rn_next, rn_ref)
    assert not slab[0].any()


def test_zero_rows_take_the_norm_clamp():
    """An all-zero mixed row: rnorm = 1 / 1e-12 in both kernels."""
    ext = _ext()
    B, N, L, d = 2, 64, 2, 512
    z = torch.zeros(B, N, L, d, device=DEV, dtype=BF)
    pos = _case(B, N, L, d)["pos"]
    out, td_next, rn_next = ext.level_mix_fwd_next(
        z, z, z[:, :, :1].contiguous(), z, None, 0, None, pos)
    _, _, rnorm = ext.consensus_fwd(out, True, None)
    assert not out.any()
    assert torch.equal(rn_next, rnorm) and torch.isfinite(rn_next).all()
    assert torch.equal(td_next[:, :, 0], pos.expand(B, N, d))


def test_ready_inputs_are_shape_checked():
    ext = _ext()
    c = _case(3, 64, 4, 512)
    with pytest.raises(RuntimeError, match="td_in"):
        _top_down(c, c["levels"], c["td"][:, :32].contiguous())
    with pytest.raises(RuntimeError, match="rnorm"):
        ext.consensus_fwd(c["levels"], True, None,
                          torch.ones(3, 64, 4, device=DEV))


# ------------------------------- model -------------------------------- #

def test_switch_defaults_on_and_follows_the_environment(monkeypatch):
    from glom_pytorch_amd.ops import functional as Fn
    levels = torch.zeros(1, 4, 3, 8)
    monkeypatch.delenv("GLOM_NO_MIX_FUSION", raising=False)
    assert Fn.MIX_FUSION is True and Fn._LoopCarry(levels).fuse
    monkeypatch.setenv("GLOM_NO_MIX_FUSION", "1")
    assert not Fn._LoopCarry(levels).fuse       # read per call
    monkeypatch.delenv("GLOM_NO_MIX_FUSION")
    U.set_switch(SWITCH, False)
    try:
        assert not Fn._LoopCarry(levels).fuse
    finally:
        U.set_switch(SWITCH, True)


@pytest.mark.parametrize("cfg,expect", [
    ("dim512", [False, True, True, True]),
    ("dim256_fallback", [False, False, False, False])])
def test_which_iterations_get_ready_inputs(cfg, expect, monkeypatch):
    """Iteration 0 has no predecessor; the last mix emits nothing."""
    ext = _ext()
    m, img = U.model_and_img(CFGS[cfg])
    ready, emits = [], []
    real_c, real_m = ext.consensus_fwd, ext.level_mix_fwd_next

    def spy_c(*a):
        ready.append(len(a) > 3 and a[3] is not None)
        return real_c(*a)

    def spy_m(*a):
        emits.append(True)
        return real_m(*a)
    monkeypatch.setattr(ext, "consensus_fwd", spy_c)
    monkeypatch.setattr(ext, "level_mix_fwd_next", spy_m)
    with torch.no_grad():
        m(img, iters=4)
    torch.cuda.synchronize()
    assert ready == expect
    assert len(emits) == 3       # asked of every mix but the last


@pytest.mark.parametrize("case", U.FORWARD_CASES)
@pytest.mark.parametrize("cfg", list(CFGS))
def test_forward_equal_with_and_without_the_fusion(cfg, case):
    U.assert_forward_equal(SWITCH, CFGS[cfg], case)


@pytest.mark.parametrize("overlap_tail", [False, True],
                         ids=["inline_tail", "overlap_tail"])
@pytest.mark.parametrize("path", list(U.BWD_PATHS))
@pytest.mark.parametrize("grad_iters,lmin", U.TRAIN_CASES, ids=U.TRAIN_IDS)
@pytest.mark.parametrize("cfg", list(CFGS))
def test_gradients_equal_with_and_without_the_fusion(
        cfg, grad_iters, lmin, path, overlap_tail, monkeypatch):
    for k in ("GLOM_BWD_FORK", "GLOM_NO_BWD_STREAMS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in U.BWD_PATHS[path].items():
        monkeypatch.setenv(k, v)
    U.assert_grads_equal(SWITCH, CFGS[cfg], grad_iters, lmin, overlap_tail)


@pytest.mark.parametrize("graph_step", [True, False],
                         ids=["captured", "eager_launch"])
@pytest.mark.parametrize("cfg", list(CFGS))
def test_trainer_equal_with_and_without_the_fusion(cfg, graph_step):
    U.assert_trainer_equal(SWITCH, CFGS[cfg], graph_step)
