"""Contrastive regularisation of GLOM level states.

The embedding of one patch column at a (high) level should agree across two
corruptions of the same image and disagree with the columns of other
images. This is the open to-do at the end of the reference's README; the
denoising objective alone lets the level embeddings collapse.

    column_contrastive_loss(a, b, temperature=0.1, negatives="other_images",
                            symmetric=False) -> fp32 scalar tensor

``a`` and ``b`` are ``(B, N, D)``: the embeddings of the same B images and N
patch columns under two views (strided slices such as ``traj[t, :, :, l]``
are fine). The loss is differentiable in both.

Semantics (the torch implementation below is the specification, the way
``islands.py`` is for the island analysis). Let ``M = B*N`` and row
``i = p*N + n``:

- Reciprocal norms ``ra_i = 1 / max(|a_i|, 1e-8)`` and ``rb_j`` likewise,
  computed in fp32 from the stored values.
- Logits ``s_ij = ra_i * rb_j * <a_i, b_j> / temperature``.
- Row ``i`` may see column ``j``:
  ``negatives="other_images"`` (default): ``j == i`` and every ``j`` of a
  different image. Other columns of the *same* image are neither positive
  nor negative -- at high levels they are supposed to be the same island.
  ``negatives="all"``: every ``j``.
- Loss ``mean_i [ logsumexp_{j allowed}(s_ij) - s_ii ]``.
- ``symmetric=True`` returns ``0.5 * (L(a, b) + L(b, a))``, composed from
  two calls.
- With ``B == 1`` and ``other_images`` only the positive is left and the
  loss is exactly 0.

The specification computes in fp32 (in fp64 for fp64 inputs) and builds the
``M x M`` logits. Dispatch follows the package rule: bf16 CUDA inputs with
``D % 8 == 0`` and ``temperature >= MIN_NATIVE_TEMPERATURE`` run the gfx950
HIP path (``ContrastFn`` in ``ops/functional.py``), which never stores the
logits, uses no atomics, is run-to-run bitwise reproducible, never
synchronises with the host (so it records into a hipGraph) and raises if
the extension is missing. Rows are read in 16-byte pieces, so an input
whose row stride is no multiple of 8 elements or whose base is not 16-byte
aligned is cloned first. Everything else (CPU, other dtypes, other ``D``,
smaller temperatures, ``GLOM_FORCE_EAGER=1``) runs the torch code.

The temperature floor exists because ``|s_ij| <= 1/temperature``: the
kernels use the fixed shift ``exp(s - 1/temperature)`` instead of an online
maximum, which makes row partial sums plain sums in a fixed order; the floor
keeps ``exp(-2/temperature)`` a normal fp32 number.
"""

from __future__ import annotations

import os

import torch

__all__ = ["column_contrastive_loss", "native_calls", "NEGATIVES",
           "MIN_NATIVE_TEMPERATURE", "EPS"]

NEGATIVES = ("other_images", "all")
MIN_NATIVE_TEMPERATURE = 0.03
EPS = 1e-8

_NATIVE_CALLS = 0


def native_calls() -> int:
    """Number of native loss evaluations (forward passes of the HIP path)
    that completed in this process; ``symmetric=True`` counts two."""
    return _NATIVE_CALLS


def _force_eager() -> bool:
    return os.environ.get("GLOM_FORCE_EAGER", "0") == "1"


# --------------------------------------------------------------------- #
# torch implementation (the specification)

def _torch_loss(a: torch.Tensor, b: torch.Tensor, temperature: float,
                negatives: str) -> torch.Tensor:
    B, N, D = a.shape
    M = B * N
    dt = torch.float64 if a.dtype == torch.float64 else torch.float32
    x = a.reshape(M, D).to(dt)
    y = b.reshape(M, D).to(dt)
    ra = 1.0 / x.norm(dim=-1).clamp_min(EPS)
    rb = 1.0 / y.norm(dim=-1).clamp_min(EPS)
    s = (x @ y.t()) * ra[:, None] * rb[None, :] / temperature
    pos = s.diagonal()
    if negatives == "other_images":
        img = torch.arange(M, device=a.device) // N
        idx = torch.arange(M, device=a.device)
        allowed = (img[:, None] != img[None, :]) | (idx[:, None] == idx[None, :])
        s = s.masked_fill(~allowed, float("-inf"))
    loss = (torch.logsumexp(s, dim=-1) - pos).mean()
    return loss.float() if dt == torch.float32 else loss


# --------------------------------------------------------------------- #
# dispatch

def _native_ok(a: torch.Tensor, b: torch.Tensor, temperature: float) -> bool:
    return (a.is_cuda and b.is_cuda
            and a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16
            and a.shape[-1] % 8 == 0 and a.numel() > 0
            and temperature >= MIN_NATIVE_TEMPERATURE
            and not _force_eager())


def _rows(x: torch.Tensor) -> torch.Tensor:
    """``(B, N, D)`` as an ``(M, D)`` matrix the kernels can read: unit
    column stride, one row stride that is a multiple of 8 elements, 16-byte
    aligned base. A view where the layout allows it, else a dense copy."""
    B, N, D = x.shape
    sb, sn, sd = x.stride()
    if ((sd == 1 or D == 1) and (B == 1 or sb == N * sn) and sn % 8 == 0
            and sn >= D and x.data_ptr() % 16 == 0):
        return x.as_strided((B * N, D), (sn, 1))
    return x.reshape(B * N, D).clone(memory_format=torch.contiguous_format)


def _native_loss(a, b, temperature, negatives):
    global _NATIVE_CALLS
    from glom_pytorch_amd.ops.functional import ContrastFn
    N = a.shape[1]
    loss = ContrastFn.apply(_rows(a), _rows(b), N, float(temperature),
                            negatives == "all")
    _NATIVE_CALLS += 1
    return loss


def column_contrastive_loss(a: torch.Tensor, b: torch.Tensor,
                            temperature: float = 0.1,
                            negatives: str = "other_images",
                            symmetric: bool = False) -> torch.Tensor:
    """InfoNCE over patch columns of two views, ``(B, N, D) x 2 -> ()``;
    see the module docstring for the exact definition."""
    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError("a and b must both be (B, N, D) with equal shapes, "
                         f"got {tuple(a.shape)} and {tuple(b.shape)}")
    if not temperature > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    if negatives not in NEGATIVES:
        raise ValueError(f"negatives must be one of {NEGATIVES}, "
                         f"got {negatives!r}")
    if a.dtype != b.dtype or a.device != b.device:
        raise ValueError("a and b must share dtype and device")
    if symmetric:
        return 0.5 * (column_contrastive_loss(a, b, temperature, negatives)
                      + column_contrastive_loss(b, a, temperature, negatives))
    if _native_ok(a, b, float(temperature)):
        return _native_loss(a, b, temperature, negatives)
    return _torch_loss(a, b, float(temperature), negatives)
