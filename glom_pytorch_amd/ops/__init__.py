"""HIP/CDNA4 op layer: loader for the in-tree gfx950 extension + autograd ops.

The extension (`_glom_hip*.so`) is built in-tree by ``setup.py build_ext
--inplace`` (PYTORCH_ROCM_ARCH=gfx950) so the binary travels with the repo
snapshot to GPU machines. On a GPU box the native path is mandatory: if a
bf16 CUDA tensor reaches ``native_forward`` and the extension cannot be
loaded, we raise instead of silently falling back to eager PyTorch.
"""

from __future__ import annotations

import glob
import importlib
import os

import torch

_EXT = None
_EXT_ERR: Exception | None = None


def _load_extension():
    global _EXT, _EXT_ERR
    if _EXT is not None:
        return _EXT
    if _EXT_ERR is not None:
        raise _EXT_ERR
    try:
        from glom_pytorch_amd.ops import _glom_hip  # built in-tree
        _EXT = _glom_hip
        return _EXT
    except ImportError as e:
        here = os.path.dirname(__file__)
        sos = glob.glob(os.path.join(here, "_glom_hip*.so"))
        _EXT_ERR = ImportError(
            f"glom_pytorch_amd HIP extension not importable ({e}). "
            f"Found candidate .so files: {sos or 'none'}. Build it in-tree with "
            f"`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace` "
            f"from the repo root. The GPU path never falls back to eager.")
        raise _EXT_ERR


def available() -> bool:
    try:
        _load_extension()
        return True
    except ImportError:
        return False


def native_forward(model, img, iters, levels=None, return_all=False,
                   grad_iters=None, overlap_tail=False, loss_level_min=None):
    """Run Glom.forward on the CDNA4 HIP engine (bf16, gfx950)."""
    from glom_pytorch_amd.ops.functional import glom_forward
    return glom_forward(model, img, iters=iters, levels=levels,
                        return_all=return_all, grad_iters=grad_iters,
                        overlap_tail=overlap_tail,
                        loss_level_min=loss_level_min)


def set_token_hoist(on: bool) -> None:
    """Token-MLP hoist (default on; ``GLOM_NO_TOKEN_HOIST=1`` turns it off):
    bottom-up group 0 reads only the tokens, so it runs in iteration 0 of a
    forward and afterwards only at steps whose backward reads its
    pre-activations. Values and gradients are bit-identical either way.
    Read once per forward."""
    from glom_pytorch_amd.ops import functional
    functional.set_token_hoist(on)


def set_mix_fusion(on: bool) -> None:
    """Level-mix fusion (default on; ``GLOM_NO_MIX_FUSION=1`` turns it off):
    the level mix also writes the next iteration's top-down input and row
    norms (dim 512; other dims keep the standalone kernels). Bit-identical
    either way. Read once per forward."""
    from glom_pytorch_amd.ops import functional
    functional.set_mix_fusion(on)


def set_bwd_merge(on: bool) -> None:
    """Backward merge (default on; ``GLOM_NO_BWD_MERGE=1`` turns it off):
    under ``loss_level_min`` one cone-aware kernel sums the four
    levels-gradient contributions of a step and prepares the previous
    step's mix gradient, the top-down backward reads that gradient in
    place, dB2 is summed once, and no zero slices are written to be read
    back; times the loss does not read get no trajectory gradient.
    Bit-identical either way. Read once per forward."""
    from glom_pytorch_amd.ops import functional
    functional.set_bwd_merge(on)


def trajectory_at(all_levels, t):
    """``all_levels[t]`` of a ``return_all`` forward, without the dense
    trajectory gradient where the forward ran under ``loss_level_min``
    (see ``ops.functional.trajectory_at``)."""
    from glom_pytorch_amd.ops import functional
    return functional.trajectory_at(all_levels, t)


def set_check_level_cone(on: bool) -> None:
    """Level-cone check mode: before each step's backward, verify with one
    host sync that the gradient is zero below the level ``loss_level_min``
    promised, and raise ``RuntimeError`` naming the iteration and level if
    not. Off by default (``GLOM_CHECK_LEVEL_CONE=1`` turns it on); cannot
    run under stream capture."""
    from glom_pytorch_amd.ops import functional
    functional.set_check_level_cone(on)
