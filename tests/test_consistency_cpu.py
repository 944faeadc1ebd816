"""Consistency term, the torch specification (``Glom._eager_step`` /
``_eager_forward`` through ``consistency._spec_forward``, here called
``consistency_forward``), against the loop-level recomputation of
``_consistency_util``; the call's contract; the helper.

The cases that need ``Glom.forward(return_consistency=)`` or the trainer
option (``ValueError`` with ``loss_level_min``, the four trainer cases) wait
for those: docs/ARCHITECTURE.md "Consistency loss"."""

import pytest
import torch

from conftest import SMALL, SMALL_BATCH, SMALL_ITERS
from _consistency_util import recompute_consistency

from glom_pytorch_amd import Glom, consistency_loss
from glom_pytorch_amd.consistency import _spec_forward as consistency_forward

CONFIGS = {"small": SMALL, "levels2": dict(SMALL, levels=2)}


def _model(name, dtype):
    torch.manual_seed(0)
    m = Glom(**CONFIGS[name]).to(dtype)
    img = torch.randn(SMALL_BATCH, 3, SMALL["image_size"],
                      SMALL["image_size"], dtype=dtype)
    return m, img


def _grads(m, loss):
    m.zero_grad(set_to_none=True)
    loss.backward()
    return {n: p.grad.clone() for n, p in m.named_parameters()}


def _mix(c):
    """A scalar that weights every entry differently."""
    w = torch.arange(1, c.numel() + 1, dtype=c.dtype).view_as(c) / c.numel()
    return (c * w).sum()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64],
                         ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_specification_equals_the_loop_level_recomputation(name, dtype):
    m, img = _model(name, dtype)
    L = m.levels
    traj, c = consistency_forward(m, img, iters=SMALL_ITERS,
                                  return_all=True)
    assert c.shape == (SMALL_ITERS, 2, L)
    assert c.dtype == dtype                  # fp32, or fp64 for fp64 models
    assert not c[:, 1, L - 1].any()
    ref = recompute_consistency(m, img, traj)
    tol = 1e-10 if dtype == torch.float64 else 2e-5
    assert ((c - ref).abs() <= tol * ref.abs()).all()
    g = _grads(m, _mix(c))
    traj2 = m(img, iters=SMALL_ITERS, return_all=True)
    g_ref = _grads(m, _mix(recompute_consistency(m, img, traj2)))
    assert set(g) == set(g_ref) and len(g) == 12
    for n in g:         # relative to the tensor's largest entry
        scale = g_ref[n].abs().max()
        assert scale > 0, n
        assert (g[n] - g_ref[n]).abs().max() <= tol * scale, n
    # the stop-gradient matters: without the detach the gradients differ
    traj3 = m(img, iters=SMALL_ITERS, return_all=True)
    g_no = _grads(m, _mix(recompute_consistency(m, img, traj3,
                                                detach=False)))
    differ = [n for n in g
              if (g[n] - g_no[n]).abs().max() > 1e-3 * g[n].abs().max()]
    assert len(differ) >= 6, differ


def test_bf16_model_gets_an_fp32_tensor():
    m, img = _model("small", torch.bfloat16)
    with torch.no_grad():
        out, c = consistency_forward(m, img, iters=2)
    assert out.dtype == torch.bfloat16 and c.dtype == torch.float32
    assert (c[:, 0] > 0).all()


def test_default_return_type_and_other_results_unaffected():
    m, img = _model("small", torch.float32)
    with torch.no_grad():
        plain = m(img, iters=SMALL_ITERS)
        assert isinstance(plain, torch.Tensor)
        out, c = consistency_forward(m, img, iters=SMALL_ITERS)
        assert torch.equal(out, plain)
        traj = m(img, iters=SMALL_ITERS, return_all=True)
        traj_c, c2 = consistency_forward(m, img, iters=SMALL_ITERS,
                                         return_all=True)
        assert torch.equal(traj_c, traj) and torch.equal(c, c2)
        # stateful levels=
        state = traj[1].clone()
        cont = m(img, iters=2, levels=state)
        cont_c, c3 = consistency_forward(m, img, iters=2, levels=state)
        assert torch.equal(cont_c, cont)
        assert torch.allclose(c3, c[1:3], rtol=1e-4, atol=0)


def test_rows_from_grad_iters_on_carry_no_gradient():
    m, img = _model("small", torch.float64)
    _, c = consistency_forward(m, img, iters=4, grad_iters=2)
    _, c_full = consistency_forward(m, img, iters=4)
    assert torch.equal(c.detach(), c_full.detach())      # same values
    g = torch.autograd.grad(c[2:].sum(), list(m.parameters()),
                            allow_unused=True, retain_graph=True)
    assert all(x is None or not x.any() for x in g)
    g = torch.autograd.grad(c[:2].sum(), list(m.parameters()))
    assert all(x.abs().sum() > 0 for x in g)


def test_helper_is_the_weighted_mean():
    torch.manual_seed(3)
    L, iters, T = 4, 5, 3
    c = torch.rand(iters, 2, L, dtype=torch.float64)
    c[:, 1, L - 1] = 0
    w = [0.5, 0.0, 2.0, 1.0]
    want = sum(w[l] * c[t, k, l] for t in range(T) for k in range(2)
               for l in range(L) if not (k == 1 and l == L - 1))
    want = want / (T * (sum(w) + sum(w[:-1])))
    assert torch.allclose(consistency_loss(c, w, upto=T), want, rtol=1e-12)
    assert torch.allclose(consistency_loss(c, torch.tensor(w), upto=T), want,
                          rtol=1e-12)
    ones = consistency_loss(c, [1.0] * L)
    assert torch.allclose(consistency_loss(c), ones, rtol=1e-12)
    assert torch.allclose(ones, c.sum() / (iters * (2 * L - 1)), rtol=1e-12)
    for bad in ([1.0] * 3, [1.0, -1.0, 1.0, 1.0], [0.0] * 4,
                torch.zeros(4), torch.tensor([1.0, -1.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            consistency_loss(c, bad)
    with pytest.raises(ValueError):
        consistency_loss(c, upto=6)
    with pytest.raises(ValueError):
        consistency_loss(c[0])


def test_level_weights_reach_only_what_the_formula_says():
    """Weight on the top level alone: c[t, 0, L-1] is the one weighted
    entry (c[t, 1, L-1] is zero). Bottom-up group L-1 reads level L-2, which
    earlier iterations' top-down group L-2 predicted, so that group's
    gradient is non-zero from the second iteration on."""
    m, img = _model("small", torch.float64)
    L, T = m.levels, 2
    m4 = m.dim * 4
    top_only = [0.0] * (L - 1) + [1.0]
    _, c = consistency_forward(m, img, iters=SMALL_ITERS, grad_iters=T)
    top = _grads(m, consistency_loss(c, top_only, upto=T))
    g_td = top["top_down.net.1.weight"]
    assert g_td[(L - 2) * m4:(L - 1) * m4].abs().sum() > 0
    # the formula: only c[:T, 0, L-1] counts, normalised by T * w_top
    _, c = consistency_forward(m, img, iters=SMALL_ITERS, grad_iters=T)
    by_hand = _grads(m, c[:T, 0, L - 1].sum() / T)
    for n in top:
        assert torch.allclose(top[n], by_hand[n], rtol=1e-10, atol=1e-300), n
    # at T = 1 nothing upstream of bottom-up group L-1 is a parameter of
    # the top-down net: its gradient is exactly zero
    _, c1 = consistency_forward(m, img, iters=SMALL_ITERS, grad_iters=1)
    g1 = _grads(m, consistency_loss(c1, top_only, upto=1))
    assert not g1["top_down.net.1.weight"].any()
    bu1 = g1["bottom_up.net.1.weight"]
    assert not bu1[:(L - 1) * m4].any() and bu1[(L - 1) * m4:].any()


def test_bad_image_shape_is_refused():
    m, img = _model("small", torch.float32)
    with pytest.raises(ValueError):
        consistency_forward(m, img[0])
