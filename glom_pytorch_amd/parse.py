"""Parse trees from islands of agreement.

GLOM represents an image as a part-whole parse tree: an island at level
``l`` is a node, and the island at level ``l+1`` that lies over it is its
parent. ``glom_pytorch_amd.islands`` finds the nodes; this module joins them
into a tree and says what vector each node stands for.

    island_parents(labels, return_overlap=False)
        -> int32 parents (*lead, L, H, W) [, int32 overlap]
    island_means(levels, labels, broadcast=False, dtype=torch.float32)
        -> (*lead, N, L, D) in dtype
    parse_tree(levels, threshold=0.9, grid=None, connectivity=4)
        -> ParseTree(labels, sizes, parents, overlap, means)
    tree_nodes(tree, index) -> [(level, root, size, parent, overlap), ...]

Semantics (the torch implementation below is the specification):

- Everything is defined on label *values*, so labels need not be canonical.
  Within one ``(lead, level)`` problem the *group* ``r`` is the set of cells
  ``n`` with ``labels[n] == r``; its results are stored at cell ``r``. A
  cell whose label is outside ``[0, N)`` belongs to no group and is ignored.
- ``island_parents``: for each level ``l < L-1`` and group ``r``, count for
  every in-range ``q`` the cells with ``labels[l] == r`` and
  ``labels[l+1] == q``. ``parents[l]`` at cell ``r`` is the ``q`` with the
  largest count (ties go to the smallest ``q``) and ``overlap[l]`` at cell
  ``r`` is that count. Every cell that is not a group key holds ``-1`` /
  ``0``, and so does a group none of whose cells has an in-range label one
  level up. The whole level ``L-1`` holds ``-1`` / ``0``.
- ``island_means``: row ``(r, l)`` holds the mean of the rows
  ``levels[n, l]`` over group ``r`` of level ``l``, accumulated in fp32,
  divided once by the group size and rounded once to ``dtype`` (``float32``
  or ``bfloat16``). With ``broadcast=False`` every other row is zero; with
  ``broadcast=True`` every cell with an in-range label holds its group's
  mean and the remaining rows are zero. A bf16 broadcast result has the
  layout of a level state and can be fed back as ``model(img, levels=...)``.

Dispatch follows the package rule. int32 CUDA labels with ``N <= 1024`` run
the gfx950 HIP kernels (``ops/csrc/parse_kernels.hip``); ``island_means``
additionally needs bf16 CUDA levels with ``D % 8 == 0``. The native path
never synchronises with the host, so it can be recorded into a hipGraph, it
sums every group in ascending cell order, so its results are bitwise
reproducible, and it raises if the extension is missing. Everything else
(CPU, fp32 levels, int64 labels, other ``D``, larger grids,
``GLOM_FORCE_EAGER=1``) runs the torch implementation on the tensor's
device.

All functions are non-differentiable: inputs are detached.
"""

from __future__ import annotations

import os
from typing import NamedTuple

import torch

from glom_pytorch_amd import islands as _islands

__all__ = ["ParseTree", "island_parents", "island_means", "parse_tree",
           "tree_nodes", "native_calls", "MAX_NATIVE_CELLS"]

MAX_NATIVE_CELLS = 1024      # PARSE_MAX_CELLS in ops/csrc/parse_kernels.h

# elements of the (problems, N, N) count table the torch vote holds at once
_VOTE_CHUNK_ELEMS = 1 << 26

_NATIVE_CALLS = 0


class ParseTree(NamedTuple):
    """``labels``, ``sizes``, ``parents``, ``overlap``: int32
    ``(*lead, L, H, W)``; ``means``: float32 ``(*lead, N, L, D)``, one row
    per island at its root cell, zero elsewhere."""
    labels: torch.Tensor
    sizes: torch.Tensor
    parents: torch.Tensor
    overlap: torch.Tensor
    means: torch.Tensor


def native_calls() -> int:
    """Number of extension calls of this module that completed in this
    process: one per native ``island_parents`` or ``island_means``. The
    island ops a ``parse_tree`` runs are counted by
    ``islands.native_calls()``."""
    return _NATIVE_CALLS


def _native(name: str, *args):
    """Run one op of the HIP extension; counted once it has returned."""
    global _NATIVE_CALLS
    from glom_pytorch_amd.ops import _load_extension
    ext = _load_extension()      # raises: no silent fallback on GPU
    out = getattr(ext, name)(*args)
    _NATIVE_CALLS += 1
    return out


def _force_eager() -> bool:
    return os.environ.get("GLOM_FORCE_EAGER", "0") == "1"


# --------------------------------------------------------------------- #
# torch implementation (the specification)

def _torch_parents(labels: torch.Tensor):
    L, H, W = labels.shape[-3:]
    N = H * W
    dev = labels.device
    lab = labels.reshape(-1, L, N).long()
    P = lab.shape[0]
    parents = torch.full((P, L, N), -1, dtype=torch.int64, device=dev)
    overlap = torch.zeros((P, L, N), dtype=torch.int64, device=dev)
    if L > 1 and P * N > 0:
        la = lab[:, :-1].reshape(-1, N)
        lb = lab[:, 1:].reshape(-1, N)
        ok = (la >= 0) & (la < N) & (lb >= 0) & (lb < N)
        # cell (r, q) of a problem's N x N count table; N*N is a dump slot
        cell = torch.where(ok, la * N + lb, torch.full_like(la, N * N))
        one = torch.ones_like(cell)
        # packed vote (count * N + (N-1-q)): its maximum over q is the
        # largest count, ties to the smallest q, whatever the order
        rank = (N - 1 - torch.arange(N, device=dev)).view(1, 1, N)
        par = torch.empty_like(la)
        ovl = torch.empty_like(la)
        step = max(1, _VOTE_CHUNK_ELEMS // (N * N))
        for s in range(0, la.shape[0], step):
            c = cell[s:s + step]
            cnt = torch.zeros((c.shape[0], N * N + 1), dtype=torch.int64,
                              device=dev).scatter_add_(1, c, one[s:s + step])
            best = (cnt[:, :N * N].view(-1, N, N) * N + rank).amax(dim=2)
            ovl[s:s + step] = best // N
            par[s:s + step] = N - 1 - best % N
        par = torch.where(ovl > 0, par, torch.full_like(par, -1))
        parents[:, :-1] = par.view(P, L - 1, N)
        overlap[:, :-1] = ovl.view(P, L - 1, N)
    return (parents.to(torch.int32).reshape(labels.shape),
            overlap.to(torch.int32).reshape(labels.shape))


def _torch_means(levels: torch.Tensor, labels: torch.Tensor,
                 broadcast: bool, dtype: torch.dtype):
    N, L, D = levels.shape[-3:]
    dev = levels.device
    x = levels.reshape(-1, N, L, D).float().permute(0, 2, 1, 3)  # (P,L,N,D)
    lab = labels.reshape(-1, L, N).long()
    P = lab.shape[0]
    ok = (lab >= 0) & (lab < N)
    slot = torch.where(ok, lab, torch.full_like(lab, N))         # N: dump
    sums = torch.zeros((P, L, N + 1, D), dtype=torch.float32, device=dev)
    sums.scatter_add_(2, slot.unsqueeze(-1).expand(P, L, N, D), x)
    size = torch.zeros((P, L, N + 1), dtype=torch.float32, device=dev)
    size.scatter_add_(2, slot, torch.ones_like(slot, dtype=torch.float32))
    # rows of empty groups hold the sum 0 and stay 0
    mean = sums[:, :, :N] / size[:, :, :N].clamp_min(1.0).unsqueeze(-1)
    if broadcast:
        at = slot.clamp_max(N - 1).unsqueeze(-1).expand(P, L, N, D)
        mean = torch.where(ok.unsqueeze(-1), mean.gather(2, at),
                           torch.zeros_like(mean))
    return mean.permute(0, 2, 1, 3).to(dtype).contiguous().reshape(
        levels.shape)


# --------------------------------------------------------------------- #
# dispatch

def _check_labels(labels: torch.Tensor) -> torch.Tensor:
    if (not isinstance(labels, torch.Tensor) or labels.dim() < 3
            or labels.dtype not in (torch.int32, torch.int64)):
        raise ValueError("labels must be an integer (*lead, L, H, W) tensor")
    return labels.detach().contiguous()


def _native_labels(labels: torch.Tensor) -> bool:
    return (labels.is_cuda and labels.dtype == torch.int32
            and labels.shape[-2] * labels.shape[-1] <= MAX_NATIVE_CELLS
            and labels.numel() > 0 and not _force_eager())


def island_parents(labels: torch.Tensor, return_overlap: bool = False):
    """Parent label of every island one level up: integer
    ``(*lead, L, H, W) -> int32`` of the same shape; with ``return_overlap``
    also the number of cells the island shares with that parent."""
    labels = _check_labels(labels)
    if _native_labels(labels):
        parents, overlap = _native("island_parents", labels)
    else:
        with torch.no_grad():
            parents, overlap = _torch_parents(labels)
    return (parents, overlap) if return_overlap else parents


def island_means(levels: torch.Tensor, labels: torch.Tensor,
                 broadcast: bool = False,
                 dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Mean level-state vector of every island: ``levels (*lead, N, L, D)``,
    ``labels (*lead, L, H, W)`` with ``H*W == N`` -> ``(*lead, N, L, D)`` in
    ``dtype``; at the island's root row, or at every member row with
    ``broadcast``."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("dtype must be torch.float32 or torch.bfloat16, "
                         f"got {dtype}")
    if levels.dim() < 3 or not levels.is_floating_point():
        raise ValueError("levels must be a floating-point (*lead, N, L, D) "
                         f"tensor, got {tuple(levels.shape)}")
    labels = _check_labels(labels)
    N, L, D = levels.shape[-3:]
    if labels.dim() != levels.dim() or labels.shape[:-3] != levels.shape[:-3]:
        raise ValueError(f"lead dimensions differ: levels "
                         f"{tuple(levels.shape)}, labels "
                         f"{tuple(labels.shape)}")
    if labels.shape[-3] != L or labels.shape[-2] * labels.shape[-1] != N:
        raise ValueError(f"labels {tuple(labels.shape)} do not cover the "
                         f"N={N} cells and L={L} levels of levels")
    if labels.device != levels.device:
        raise ValueError("levels and labels must be on the same device")
    levels = levels.detach().contiguous()
    if (_native_labels(labels) and levels.dtype == torch.bfloat16
            and D % 8 == 0 and levels.numel() > 0):
        if levels.data_ptr() % 16:       # the kernel reads rows in 16 B pieces
            levels = levels.clone()
        return _native("island_means", levels, labels, bool(broadcast),
                       dtype == torch.bfloat16)
    with torch.no_grad():
        return _torch_means(levels, labels, bool(broadcast), dtype)


def parse_tree(levels: torch.Tensor, threshold: float = 0.9, grid=None,
               connectivity: int = 4) -> ParseTree:
    """Islands of level states ``(*lead, N, L, D)`` joined into a tree: the
    labels and sizes of ``glom_pytorch_amd.islands``, every island's parent
    and overlap one level up, and its fp32 mean vector at its root row."""
    labels = _islands.island_labels(levels, threshold=threshold, grid=grid,
                                    connectivity=connectivity)
    sizes = _islands.island_sizes(labels)
    parents, overlap = island_parents(labels, return_overlap=True)
    means = island_means(levels, labels)
    return ParseTree(labels, sizes, parents, overlap, means)


def tree_nodes(tree: ParseTree, index=()) -> list:
    """Nodes of one lead index of a tree as plain
    ``(level, root, size, parent, overlap)`` tuples, by level and root.
    Copies to the host, so it synchronises."""
    index = tuple(index) if isinstance(index, (tuple, list)) else (index,)
    if len(index) != tree.labels.dim() - 3:
        raise ValueError(f"index {index} does not select one of the lead "
                         f"dimensions {tuple(tree.labels.shape[:-3])}")
    sizes = tree.sizes[index].flatten(1).cpu()
    parents = tree.parents[index].flatten(1).cpu()
    overlap = tree.overlap[index].flatten(1).cpu()
    nodes = []
    for l in range(sizes.shape[0]):
        for r in torch.nonzero(sizes[l]).flatten().tolist():
            nodes.append((l, r, int(sizes[l, r]), int(parents[l, r]),
                          int(overlap[l, r])))
    return nodes
