"""Cross-check against the upstream glom-pytorch package.

The upstream results are stored under tests/golden/ (recorded on CPU in fp32
by scripts/make_reference_golden.py from an upstream checkout): upstream's
own state_dict, the inputs, and upstream's outputs and parameter gradients.
The tests load that state_dict into our model with strict=True (so key names
and shapes must match upstream's exactly) and compare what we compute with
what upstream computed, at the tolerances of a live side-by-side run.
"""

import os

import numpy as np
import pytest
import torch

from glom_pytorch_amd import Glom

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BASE = dict(dim=64, levels=3, image_size=32, patch_size=8)


@pytest.fixture(scope="module")
def fwd():
    with np.load(os.path.join(GOLDEN, "upstream_forward.npz")) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.fixture(scope="module")
def grads():
    with np.load(os.path.join(GOLDEN, "upstream_grads.npz")) as z:
        return {k[len("g/"):]: torch.from_numpy(z[k]) for k in z.files}


def _upstream_state(fwd, cfg_idx):
    """Upstream's state_dict for recorded config `cfg_idx`: the shared
    weights plus that config's buffers (the locality mask)."""
    sd = {k[len("w/"):]: v for k, v in fwd.items() if k.startswith("w/")}
    pre = f"c{cfg_idx}/buf/"
    sd.update({k[len(pre):]: v for k, v in fwd.items() if k.startswith(pre)})
    return sd


@pytest.mark.parametrize("idx,kw", [
    (0, dict(dim=64, levels=3, image_size=32, patch_size=8)),
    (1, dict(dim=64, levels=3, image_size=32, patch_size=8,
             consensus_self=True)),
    (2, dict(dim=64, levels=3, image_size=32, patch_size=8,
             local_consensus_radius=2)),
], ids=["kw0", "kw1", "kw2"])
def test_forward_matches_upstream(fwd, idx, kw):
    ours = Glom(**kw)
    ours.load_state_dict(_upstream_state(fwd, idx), strict=True)
    img = fwd["img"]
    for it in (1, 3):
        a = ours(img, iters=it)
        b = fwd[f"c{idx}/out{it}"]
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), \
            (a - b).abs().max().item()
    a = ours(img, iters=3, return_all=True)
    b = fwd[f"c{idx}/all3"]
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)


def test_stateful_matches_upstream(fwd):
    ours = Glom(**BASE)
    ours.load_state_dict(_upstream_state(fwd, 0), strict=True)
    img1, img2 = fwd["img"], fwd["img2"]
    la = ours(img2, iters=2, levels=ours(img1, iters=3))
    lb = fwd["stateful/out"]
    assert torch.allclose(la, lb, rtol=1e-5, atol=1e-6)


def test_gradients_match_upstream(fwd, grads):
    ours = Glom(**BASE)
    ours.load_state_dict(_upstream_state(fwd, 0), strict=True)

    out_a = ours(fwd["img"], iters=3, return_all=True)
    # loss over the full trajectory reaches every parameter
    out_a.pow(2).mean().backward()
    ours_named = dict(ours.named_parameters())
    assert set(ours_named) == set(grads)
    for n, p in ours_named.items():
        q = grads[n]
        assert p.grad is not None, n
        assert torch.allclose(p.grad, q, rtol=1e-4, atol=1e-7), \
            (n, (p.grad - q).abs().max().item())
