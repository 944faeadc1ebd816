"""The level-cone arithmetic against dense autograd on the eager path.

``level_cone_lo(loss_level_min, grad_iters, t)`` claims that, for a loss on
trajectory time ``grad_iters`` at levels >= ``loss_level_min``, the gradient
arriving at iteration t is zero in every level below it. Here autograd
computes all the zeros: the gradient of each iteration's output is kept and
its level slices are checked both ways (zero below, non-zero from lo_t up,
so the bound is tight and not merely safe)."""

import pytest
import torch

from glom_pytorch_amd import Glom
from glom_pytorch_amd.ops.functional import level_cone_lo


def _step_output_grads(levels, grad_iters, loss_levels, iters):
    torch.manual_seed(0)
    m = Glom(dim=16, levels=levels, image_size=8, patch_size=4)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p) * 0.3)
    img = torch.randn(2, 3, 8, 8)
    outs = []
    step = m._eager_step

    def recording_step(bottom, lv, pos):
        out = step(bottom, lv, pos)
        if out.requires_grad:
            out.retain_grad()
        outs.append(out)
        return out
    m._eager_step = recording_step
    traj = m._eager_forward(img, iters, None, True, grad_iters,
                            loss_level_min=loss_levels.start)
    traj[grad_iters][:, :, loss_levels].pow(2).sum().backward()
    assert len(outs) == iters
    return outs


@pytest.mark.parametrize("levels,grad_iters,lmin", [
    (4, 5, 3), (4, 3, 3), (4, 5, 1), (4, 2, 2),
    (2, 3, 1), (2, 1, 1), (2, 3, 0),     # levels=2: one top-down group
])
def test_zero_level_slices_match_lo_t(levels, grad_iters, lmin):
    iters = grad_iters + 1
    outs = _step_output_grads(levels, grad_iters, slice(lmin, levels), iters)
    for t in range(grad_iters):
        lo = level_cone_lo(lmin, grad_iters, t)
        assert 0 <= lo <= lmin
        g = outs[t].grad                     # (b, n, L, d)
        live = [bool(g[:, :, l].ne(0).any()) for l in range(levels)]
        assert live == [l >= lo for l in range(levels)], (t, lo, live)
    # iterations >= grad_iters ran without a graph
    assert not outs[grad_iters].requires_grad


def test_lo_t_table_of_the_headline_recipe():
    # L = 6, decode at t = 7: iterations 6 .. 0
    assert [level_cone_lo(5, 7, t) for t in range(6, -1, -1)] == \
        [5, 4, 3, 2, 1, 0, 0]


def test_forward_argument_checks():
    m = Glom(dim=16, levels=3, image_size=8, patch_size=4)
    img = torch.randn(1, 3, 8, 8)
    # the eager path accepts and ignores the hint
    a = m(img, iters=3, grad_iters=2, loss_level_min=2)
    b = m(img, iters=3, grad_iters=2)
    assert torch.equal(a, b)
    from glom_pytorch_amd.ops.functional import glom_forward
    with pytest.raises(ValueError, match="requires grad_iters"):
        glom_forward(m, img, 3, loss_level_min=2)
    with pytest.raises(ValueError, match="level index"):
        glom_forward(m, img, 3, grad_iters=2, loss_level_min=3)
