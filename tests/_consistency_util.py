"""Loop-level recomputation of the consistency tensor, independent of
``Glom._eager_step``: explicit loops over iterations and levels, reading the
returned trajectory and the model's weights. The target of iteration t is
the trajectory's state t + 1, with this file's own ``.detach()``."""

import math

import torch


def _patch_tokens(model, img):
    p = model.patch_size
    b, c, H, W = img.shape
    h, w = H // p, W // p
    x = img.reshape(b, c, h, p, w, p).permute(0, 2, 4, 3, 5, 1)
    x = x.reshape(b, h * w, p * p * c)                # (p1 p2 c), as the model
    lin = model.image_to_tokens[1]
    return x @ lin.weight.t() + lin.bias


def _mlp(ff, g, x):
    """Group g of a GroupedFeedForward on (b, n, d) rows."""
    d, m = ff.dim, ff.dim * ff.mult
    w1 = ff.net[1].weight[g * m:(g + 1) * m, :, 0]
    b1 = ff.net[1].bias[g * m:(g + 1) * m]
    w2 = ff.net[3].weight[g * d:(g + 1) * d, :, 0]
    b2 = ff.net[3].bias[g * d:(g + 1) * d]
    h = x @ w1.t() + b1
    h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return h @ w2.t() + b2


def recompute_consistency(model, img, traj, detach=True):
    """(iters, 2, L) from ``traj``, the ``return_all`` trajectory of the model
    (with its autograd graph). Independent of the model's code for the
    per-step predictions, the distances and the detach; not for the
    recurrence: the inputs of every step are the model's own trajectory, and
    gradient reaches earlier iterations through that graph.
    ``detach=False`` lets gradient into the target: the variant whose
    gradients must differ."""
    iters = traj.shape[0] - 1
    L = model.levels
    ct = torch.promote_types(traj.dtype, torch.float32)
    tokens = _patch_tokens(model, img)
    pos = model.pos_emb.weight                         # (n, d)
    rows = []
    for t in range(iters):
        x, nxt = traj[t], traj[t + 1]
        row = [[None] * L, [None] * L]
        for l in range(L):
            tgt = nxt[:, :, l]
            if detach:
                tgt = tgt.detach()
            tgt = tgt.to(ct)
            below = tokens if l == 0 else x[:, :, l - 1]
            bu = _mlp(model.bottom_up, l, below)
            row[0][l] = (bu.to(ct) - tgt).pow(2).mean()
            if l < L - 1:
                td = _mlp(model.top_down, l, x[:, :, l + 1] + pos)
                row[1][l] = (td.to(ct) - tgt).pow(2).mean()
            else:
                row[1][l] = torch.zeros((), dtype=ct)
        rows.append(torch.stack([torch.stack(r) for r in row]))
    return torch.stack(rows)
