"""Token-MLP hoist: bottom-up group 0 reads `tokens`, not `levels`, so one
forward computes it once (iteration 0) and later iterations run groups
1..G-1 only, unless their backward reads group 0's pre-activations.

Nothing may move a bit: every comparison is ``torch.equal`` between the
switch on and off (or the op with and without "group 0 done") in the same
build. The remaining groups must keep the kernels the full call gives them
(gates judged by the full group count), which the dispatch-pinning shapes
check at the smallest sizes where 6 against 5 groups would flip a gate:
  nt5p up-projection    B=4  (M=1024): 8*2*6 = 96 tiles, the minimum; 80
  nt8p down-projection  B=24 (M=6144): 2*24*6 = 288 tiles (min 256); 240
"""

import functools

import pytest
import torch

import _loop_invariant_util as U
from _loop_invariant_util import BF, DEV, MODEL256

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

SWITCH = "set_token_hoist"


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


@functools.lru_cache(maxsize=None)
def _ff_inputs(B, N, L, d):
    m4 = 4 * d
    g = torch.Generator(device=DEV).manual_seed(11 + B + L)

    def rn(*s, scale=1.0):
        return (torch.randn(*s, device=DEV, generator=g) * scale).to(BF)
    return dict(tokens=rn(B, N, d), levels=rn(B, N, L, d),
                w1=rn(L * m4, d, scale=0.04), b1=rn(L * m4),
                w2=rn(L * d, m4, scale=0.04), b2=rn(L * d))


def _bottom_up(c, save_for_bwd, group0_done):
    return _ext().grouped_ff_fwd(c["tokens"], c["levels"], None, c["w1"],
                                 c["b1"], c["w2"], c["b2"], 0, save_for_bwd,
                                 group0_done)


def _assert_groups_from_1_equal(c, save_for_bwd, what):
    Y, Hpre, Hact, _ = _bottom_up(c, save_for_bwd, True)
    Y0, Hpre0, Hact0, _ = _bottom_up(c, save_for_bwd, False)
    torch.cuda.synchronize()
    assert Y.shape == Y0.shape and Hact.shape == Hact0.shape, what
    assert Hpre.shape == Hpre0.shape, what
    assert torch.equal(Y[:, :, 1:], Y0[:, :, 1:]), what
    assert torch.equal(Hact[1:], Hact0[1:]), what
    if save_for_bwd:
        assert Hpre.numel() > 0 and torch.equal(Hpre[1:], Hpre0[1:]), what
    else:
        assert Hpre.numel() == 0, what
    assert Y0[:, :, 1:].float().abs().sum() > 0, what


# ------------------------------ 1. op level --------------------------- #

@pytest.mark.parametrize("save_for_bwd", [True, False])
@pytest.mark.parametrize("L", [4, 2])
def test_grouped_ff_fwd_without_group0(L, save_for_bwd):
    c = _ff_inputs(2, 256, L, 256)
    _assert_groups_from_1_equal(c, save_for_bwd, (L, save_for_bwd))


def test_group0_done_is_bottom_up_only():
    ext = _ext()
    c = _ff_inputs(2, 256, 4, 256)
    pos = torch.zeros(256, 256, device=DEV, dtype=BF)
    with pytest.raises(RuntimeError, match="group0_done"):
        ext.grouped_ff_fwd(None, c["levels"], pos, c["w1"][:3 * 1024],
                           c["b1"][:3 * 1024], c["w2"][:3 * 256],
                           c["b2"][:3 * 256], 1, True, True)


@pytest.mark.parametrize("L", [4, 2])
def test_level_mix_reads_level0_from_the_kept_tensor(L):
    ext = _ext()
    B, N, d = 2, 256, 256
    g = torch.Generator(device=DEV).manual_seed(21)

    def rn(*s):
        return torch.randn(*s, device=DEV, generator=g).to(BF)
    levels, bu, cons = rn(B, N, L, d), rn(B, N, L, d), rn(B, N, L, d)
    td = rn(B, N, L - 1, d)
    ref = ext.level_mix_fwd(levels, bu, td, cons)
    # a later iteration's Y: slice 0 unwritten (here: poisoned)
    later = bu.clone()
    later[:, :, 0] = float("nan")
    strided = bu[:, :, 0, :]                   # iteration 0's Y, stride L*d
    compact = strided.contiguous()             # stride d
    for bu0 in (strided, compact):
        got = ext.level_mix_fwd(levels, later, td, cons, None, 0, bu0)
        assert torch.equal(got, ref), bu0.stride()
    # into a trajectory slab as well
    slab = torch.zeros(3, B, N, L, d, device=DEV, dtype=BF)
    got = ext.level_mix_fwd(levels, later, td, cons, slab, 2, strided)
    assert torch.equal(slab[2], ref) and torch.equal(got, ref)
    assert not slab[:2].any()
    with pytest.raises(RuntimeError, match="bu0"):
        ext.level_mix_fwd(levels, later, td, cons, None, 0,
                          bu[:, :, 0, :d // 2])


# -------------------------- 2. dispatch pinning ----------------------- #

@pytest.mark.parametrize("save_for_bwd", [True, False])
@pytest.mark.parametrize("B", [4, 24], ids=["nt5p_gate", "nt8p_gate"])
def test_five_groups_keep_the_six_group_kernels(B, save_for_bwd):
    """Outputs only: another kernel for the up- or down-projection would
    change the f32 summation order and with it the bits."""
    c = _ff_inputs(B, 256, 6, 512)
    _assert_groups_from_1_equal(c, save_for_bwd, (B, save_for_bwd))


# ------------------------------ 3. model ------------------------------ #

def test_switches_default_on_and_follow_the_environment(monkeypatch):
    from glom_pytorch_amd.ops import functional as Fn
    levels = torch.zeros(1, 4, 3, 8)
    monkeypatch.delenv("GLOM_NO_TOKEN_HOIST", raising=False)
    assert Fn.TOKEN_HOIST is True and Fn._LoopCarry(levels).hoist
    monkeypatch.setenv("GLOM_NO_TOKEN_HOIST", "1")
    assert not Fn._LoopCarry(levels).hoist      # read per call
    monkeypatch.delenv("GLOM_NO_TOKEN_HOIST")
    U.set_switch(SWITCH, False)
    try:
        assert not Fn._LoopCarry(levels).hoist
    finally:
        U.set_switch(SWITCH, True)


def test_the_hoist_really_skips_group0(monkeypatch):
    """10 of 12 iterations in the headline recipe; here: iterations 1.. of a
    no-grad forward ask for 'group 0 done', iteration 0 does not."""
    ext = _ext()
    m, img = U.model_and_img(MODEL256)
    seen = []
    real = ext.grouped_ff_fwd

    def spy(*a):
        if a[7] == 0:
            seen.append(bool(a[9]) if len(a) > 9 else False)
        return real(*a)
    monkeypatch.setattr(ext, "grouped_ff_fwd", spy)
    with torch.no_grad():
        m(img, iters=4)
    torch.cuda.synchronize()
    assert seen == [False, True, True, True]


@pytest.mark.parametrize("case", U.FORWARD_CASES)
def test_forward_equal_with_and_without_the_hoist(case):
    U.assert_forward_equal(SWITCH, MODEL256, case)


@pytest.mark.parametrize("overlap_tail", [False, True],
                         ids=["inline_tail", "overlap_tail"])
@pytest.mark.parametrize("path", list(U.BWD_PATHS))
@pytest.mark.parametrize("grad_iters,lmin", U.TRAIN_CASES, ids=U.TRAIN_IDS)
def test_gradients_equal_with_and_without_the_hoist(
        grad_iters, lmin, path, overlap_tail, monkeypatch):
    for k in ("GLOM_BWD_FORK", "GLOM_NO_BWD_STREAMS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in U.BWD_PATHS[path].items():
        monkeypatch.setenv(k, v)
    U.assert_grads_equal(SWITCH, MODEL256, grad_iters, lmin, overlap_tail)


@pytest.mark.parametrize("graph_step", [True, False],
                         ids=["captured", "eager_launch"])
def test_trainer_equal_with_and_without_the_hoist(graph_step):
    U.assert_trainer_equal(SWITCH, MODEL256, graph_step)
