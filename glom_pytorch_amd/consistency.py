"""Consistency regularisation (Hinton, arXiv:2102.12627, section 3): train
the bottom-up and top-down networks so that each one's prediction for a level
agrees with the consensus the column settles on at the next time step.

The quantity is ``c``, the per-iteration, per-network, per-level mean squared
distances, of shape
``(iters, 2, L)`` (row 0 bottom-up, row 1 top-down; ``c[:, 1, L-1]`` is zero
because the top level has no top-down prediction). Entries are kept per level
so that the caller can weight the "top-ish" levels in plain torch;
``consistency_loss`` is that weighted mean. The paper notes that the term
alone collapses the embeddings and pairs it with a contrastive one
(``glom_pytorch_amd.contrast``).

Status: preparatory. Only the torch specification exists
(``Glom._eager_step(..., consistency=True)``), reached through the private
``_spec_forward`` below, which always runs the eager path. ``Glom.forward``
has no keyword for the term and the HIP engine does not compute it; both are
open, together with the trainer option (docs/ARCHITECTURE.md "Consistency
loss" says why). ``consistency_loss`` is public and final.
"""

from __future__ import annotations

import torch


def _spec_forward(model, img: torch.Tensor, iters: int | None = None,
                  levels: torch.Tensor | None = None,
                  return_all: bool = False, grad_iters: int | None = None):
    """The specification of the consistency tensor; private until
    ``Glom.forward`` takes the keyword. Returns ``(out, c)``: ``out`` is what
    ``model(img, iters, levels, return_all, grad_iters=grad_iters)`` returns
    on the eager path, ``c`` the ``(iters, 2, L)`` consistency tensor. For
    iteration ``t`` with bottom-up prediction ``bu``, top-down prediction
    ``td`` and mixed result ``new``::

        tgt        = new.detach()
        c[t, 0, l] = mean over (B, N, D) of (bu[:, :, l] - tgt[:, :, l])**2
        c[t, 1, l] = the same for td, l < L - 1;   c[t, 1, L-1] = 0

    evaluated in fp32 (fp64 for an fp64 model). Gradient flows into the two
    predictions, and through them into the weights, the tokens, ``pos_emb``
    and the earlier iterations, never into the target. Rows ``t >=
    grad_iters`` carry no gradient."""
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"expected image batch (b, 3, H, W), got "
                         f"{tuple(img.shape)}")
    iters = iters if iters is not None else 2 * model.levels
    return model._eager_forward(img, iters, levels, return_all, grad_iters,
                                None, True)


def consistency_loss(c: torch.Tensor, level_weights=None,
                     upto: int | None = None) -> torch.Tensor:
    """``sum_{t<T,k,l} w_l c[t,k,l] / (T * sum_{k,l defined} w_l)``.

    ``c``: the ``(iters, 2, L)`` consistency tensor. ``level_weights``: ``L``
    non-negative numbers (a sequence or a 1-D tensor, read on the host),
    default all 1, with a positive weight on at least one defined entry.
    ``upto``: ``T``, the number of leading iterations that count (default
    all); only rows ``< T`` are read. "Defined" entries are all ``(0, l)``,
    and ``(1, l)`` for ``l < L - 1``; ``c[:, 1, L-1]`` is zero by
    construction, so weighting it changes nothing."""
    if c.dim() != 3 or c.shape[1] != 2:
        raise ValueError(f"expected c of shape (iters, 2, L), got "
                         f"{tuple(c.shape)}")
    iters, _, L = c.shape
    T = iters if upto is None else int(upto)
    if not 1 <= T <= iters:
        raise ValueError(f"upto must be in 1..{iters}")
    if level_weights is None:
        return c[:T].sum() / (T * (2 * L - 1))
    if isinstance(level_weights, torch.Tensor):
        level_weights = level_weights.reshape(-1).tolist()
    ws = [float(x) for x in level_weights]
    if len(ws) != L or any(not x >= 0 for x in ws):
        raise ValueError(f"level_weights must be {L} non-negative numbers")
    denom = T * (2 * sum(ws) - ws[-1])
    if not denom > 0:
        raise ValueError("level_weights leave no defined entry")
    w = torch.tensor(ws, dtype=c.dtype, device=c.device)
    return (c[:T] * w).sum() / denom
