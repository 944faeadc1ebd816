"""Islands of agreement in GLOM level states.

GLOM's level states are meant to be inspected for *islands*: groups of
neighbouring patch columns whose embedding at one level is nearly the same
vector. This module turns level states ``(*lead, N, L, D)`` -- a single
state ``(B, N, L, D)`` or the ``return_all=True`` trajectory
``(T+1, B, N, L, D)`` -- into per-level island labels on the patch grid.

    edge_agreement(levels, grid=None, connectivity=4)
        -> float32 (*lead, L, C, H, W)
    labels_from_agreement(agreement, threshold, connectivity=4)
        -> int32 (*lead, L, H, W)
    island_labels(levels, threshold=0.9, grid=None, connectivity=4,
                  return_agreement=False) -> labels [, agreement]
    island_sizes(labels) -> int32 (*lead, L, H, W)
    island_count(labels) -> int32 (*lead, L)

Semantics (the torch implementation below is the specification, the way
``Glom._eager_forward`` is for the model):

- Agreement is the cosine ``<a,b> / (max(|a|,1e-8) * max(|b|,1e-8))`` of two
  neighbouring cells' vectors at one level, computed in fp32 from the
  stored values.
- Edge channels: ``C=2`` for ``connectivity=4``, ``C=4`` for
  ``connectivity=8``. ``c=0`` right ``(h,w)-(h,w+1)``, ``c=1`` down
  ``(h,w)-(h+1,w)``, ``c=2`` down-right ``(h,w)-(h+1,w+1)``, ``c=3``
  down-left ``(h,w)-(h+1,w-1)``. The value is stored at ``(h,w)``.
- An edge that would leave the grid stores ``0.0`` and is ignored by the
  labelling structurally, whatever the threshold. Rows do not wrap around.
- An edge is kept iff ``agreement >= threshold``, compared in fp32 (the
  threshold is rounded to fp32) on exactly the value that is returned.
- Islands are the connected components of the kept-edge graph per
  ``(*lead, level)``. A cell's label is the smallest linear index ``h*W+w``
  in its component, so labels are canonical and native and torch results
  compare with ``==``.
- ``island_sizes`` holds the island size at the island's root cell (the one
  whose label is its own index) and 0 elsewhere; ``island_count`` is the
  number of root cells.

Dispatch follows the package rule. bf16 CUDA levels with ``D % 8 == 0`` and
``N <= 1024`` run the gfx950 HIP kernels (``ops/csrc/island_kernels.hip``);
so do fp32 CUDA agreement tensors and int32 CUDA labels with ``N <= 1024``.
The native path never synchronises with the host, so it can be recorded
into a hipGraph, and it raises if the extension is missing. Everything else
(CPU, fp32 levels, other ``D``, larger grids, ``GLOM_FORCE_EAGER=1``) runs
the torch implementation on the tensor's device.

All functions are non-differentiable: inputs are detached.
"""

from __future__ import annotations

import math
import os

import torch

__all__ = ["edge_agreement", "labels_from_agreement", "island_labels",
           "island_sizes", "island_count", "native_calls", "MAX_NATIVE_CELLS"]

MAX_NATIVE_CELLS = 1024      # ISLAND_MAX_CELLS in ops/csrc/island_kernels.h
EPS = 1e-8

# forward edge channels: (dh, dw)
_EDGES = ((0, 1), (1, 0), (1, 1), (1, -1))

_NATIVE_CALLS = 0


def native_calls() -> int:
    """Number of extension calls that completed in this process: one per
    native ``edge_agreement``, ``labels_from_agreement``, ``island_sizes``
    or ``island_count`` (so two per native ``island_labels``)."""
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


def _channels(connectivity: int) -> int:
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    return 2 if connectivity == 4 else 4


def _grid(n: int, grid) -> tuple[int, int]:
    if grid is None:
        side = math.isqrt(n)
        grid = (side, side)
    h, w = int(grid[0]), int(grid[1])
    if h < 1 or w < 1 or h * w != n:
        raise ValueError(f"grid {tuple(grid)} does not cover N={n} cells")
    return h, w


def _slices(dh: int, dw: int, H: int, W: int):
    """Index slices of the cells (h,w) whose (dh,dw) edge stays in the grid,
    and of their neighbours (h+dh, w+dw)."""
    a = (slice(0, H - dh), slice(max(0, -dw), W - max(0, dw)))
    b = (slice(dh, H), slice(max(0, dw), W + min(0, dw)))
    return a, b


# --------------------------------------------------------------------- #
# torch implementation (the specification)

def _torch_agreement(levels: torch.Tensor, H: int, W: int, C: int):
    lead = levels.shape[:-3]
    L, D = levels.shape[-2:]
    x = levels.reshape(-1, H, W, L, D).float()
    norm = x.norm(dim=-1).clamp_min(EPS)                    # (P, H, W, L)
    out = x.new_zeros((x.shape[0], L, C, H, W))
    for c in range(C):
        a, b = _slices(*_EDGES[c], H, W)
        if a[0].stop <= a[0].start or a[1].stop <= a[1].start:
            continue
        dot = (x[:, a[0], a[1]] * x[:, b[0], b[1]]).sum(-1)
        cos = dot / (norm[:, a[0], a[1]] * norm[:, b[0], b[1]])
        out[:, :, c, a[0], a[1]] = cos.permute(0, 3, 1, 2)
    return out.reshape(*lead, L, C, H, W)


def _torch_labels(agreement: torch.Tensor, threshold: float):
    lead = agreement.shape[:-3]
    C, H, W = agreement.shape[-3:]
    N = H * W
    dev = agreement.device
    agr = agreement.reshape(-1, C, H, W).float()
    thr = torch.tensor(float(threshold), dtype=torch.float32, device=dev)
    keep = agr >= thr
    idx = torch.arange(N, device=dev).view(H, W)
    ea, eb, kept = [], [], []
    for c in range(C):
        a, b = _slices(*_EDGES[c], H, W)
        ea.append(idx[a[0], a[1]].reshape(-1))
        eb.append(idx[b[0], b[1]].reshape(-1))
        kept.append(keep[:, c, a[0], a[1]].reshape(keep.shape[0], -1))
    ea, eb, kept = torch.cat(ea), torch.cat(eb), torch.cat(kept, dim=1)

    lab = idx.reshape(1, N).repeat(agr.shape[0], 1)
    if ea.numel() and lab.numel():
        while True:
            # hook: every kept edge whose endpoints sit in different trees
            # hangs the larger root under the smaller (labels are roots here)
            ra, rb = lab[:, ea], lab[:, eb]
            lo, hi = torch.minimum(ra, rb), torch.maximum(ra, rb)
            span = kept & (lo != hi)
            if not bool(span.any()):
                break
            lab = lab.scatter_reduce(1, torch.where(span, hi, lo), lo,
                                     "amin", include_self=True)
            # pointer jumping until every cell points at its root again
            while True:
                nxt = lab.gather(1, lab)
                if torch.equal(nxt, lab):
                    break
                lab = nxt
    return lab.to(torch.int32).reshape(*lead, H, W)


def _torch_sizes(labels: torch.Tensor):
    H, W = labels.shape[-2:]
    N = H * W
    lab = labels.reshape(-1, N).long()
    sizes = torch.zeros_like(lab).scatter_add_(1, lab, torch.ones_like(lab))
    return sizes.to(torch.int32).reshape(labels.shape)


def _torch_count(labels: torch.Tensor):
    H, W = labels.shape[-2:]
    idx = torch.arange(H * W, device=labels.device).view(H, W)
    return (labels == idx).sum(dim=(-2, -1)).to(torch.int32)


# --------------------------------------------------------------------- #
# dispatch

def _native_levels(levels: torch.Tensor, n: int) -> bool:
    return (levels.is_cuda and levels.dtype == torch.bfloat16
            and levels.shape[-1] % 8 == 0 and n <= MAX_NATIVE_CELLS
            and levels.numel() > 0 and not _force_eager())


def _native_grid(t: torch.Tensor, dtype: torch.dtype) -> bool:
    return (t.is_cuda and t.dtype == dtype
            and t.shape[-2] * t.shape[-1] <= MAX_NATIVE_CELLS
            and t.numel() > 0 and not _force_eager())


def edge_agreement(levels: torch.Tensor, grid=None, connectivity: int = 4,
                   ) -> torch.Tensor:
    """Cosine agreement of every cell with its forward grid neighbours:
    ``(*lead, N, L, D) -> float32 (*lead, L, C, H, W)``."""
    C = _channels(connectivity)
    if levels.dim() < 3:
        raise ValueError("levels must be (*lead, N, L, D), got "
                         f"{tuple(levels.shape)}")
    H, W = _grid(levels.shape[-3], grid)
    levels = levels.detach().contiguous()
    if _native_levels(levels, H * W):
        if levels.data_ptr() % 16:       # the kernel reads rows in 16 B pieces
            levels = levels.clone()
        return _native("island_agreement", levels, H, W, connectivity)
    with torch.no_grad():
        return _torch_agreement(levels, H, W, C)


def labels_from_agreement(agreement: torch.Tensor, threshold: float,
                          connectivity: int = 4) -> torch.Tensor:
    """Connected components of the edges with ``agreement >= threshold``:
    ``(*lead, L, C, H, W) -> int32 (*lead, L, H, W)``."""
    C = _channels(connectivity)
    if agreement.dim() < 4 or agreement.shape[-3] != C:
        raise ValueError(f"agreement must be (*lead, L, {C}, H, W) for "
                         f"connectivity={connectivity}, got "
                         f"{tuple(agreement.shape)}")
    agreement = agreement.detach().contiguous()
    if _native_grid(agreement, torch.float32):
        return _native("island_labels", agreement, float(threshold))
    with torch.no_grad():
        return _torch_labels(agreement, threshold)


def island_labels(levels: torch.Tensor, threshold: float = 0.9, grid=None,
                  connectivity: int = 4, return_agreement: bool = False):
    """Island labels of level states: ``(*lead, N, L, D) -> int32
    (*lead, L, H, W)``; with ``return_agreement`` also the agreement the
    labels were decided on."""
    agreement = edge_agreement(levels, grid=grid, connectivity=connectivity)
    labels = labels_from_agreement(agreement, threshold,
                                   connectivity=connectivity)
    return (labels, agreement) if return_agreement else labels


def _check_labels(labels: torch.Tensor):
    if labels.dim() < 2 or labels.dtype not in (torch.int32, torch.int64):
        raise ValueError("labels must be an integer (*lead, H, W) tensor")
    return labels.detach().contiguous()


def island_sizes(labels: torch.Tensor) -> torch.Tensor:
    """Island size at each island's root cell, 0 elsewhere."""
    labels = _check_labels(labels)
    if _native_grid(labels, torch.int32):
        return _native("island_sizes", labels, True, False)[0]
    with torch.no_grad():
        return _torch_sizes(labels)


def island_count(labels: torch.Tensor) -> torch.Tensor:
    """Number of islands per ``(*lead, level)``."""
    labels = _check_labels(labels)
    if _native_grid(labels, torch.int32):
        return _native("island_sizes", labels, False, True)[1]
    with torch.no_grad():
        return _torch_count(labels)
