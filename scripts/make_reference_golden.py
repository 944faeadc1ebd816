#!/usr/bin/env python3
"""Record the upstream glom-pytorch results that tests/test_reference_parity.py
compares against, so the suite needs no upstream checkout at test time.

    python scripts/make_reference_golden.py /path/to/glom-pytorch

Writes tests/golden/upstream_forward.npz (upstream-initialised weights,
inputs, upstream outputs for every tested config) and
tests/golden/upstream_grads.npz (upstream parameter gradients). CPU, fp32.
"""

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

BASE = dict(dim=64, levels=3, image_size=32, patch_size=8)
# order matters: tests index the recorded outputs by position
CONFIGS = [dict(), dict(consensus_self=True), dict(local_consensus_radius=2)]


def main(upstream):
    sys.path.insert(0, upstream)
    from glom_pytorch import Glom as RefGlom

    torch.manual_seed(0)
    weights = RefGlom(**BASE).state_dict()
    img = torch.randn(2, 3, 32, 32)
    img2 = torch.randn(2, 3, 32, 32)

    fwd = {"img": img.numpy(), "img2": img2.numpy()}
    for k, v in weights.items():
        fwd["w/" + k] = v.numpy()

    for i, extra in enumerate(CONFIGS):
        ref = RefGlom(**BASE, **extra)
        # buffers (the locality mask) are config-derived, not weights
        ref.load_state_dict(weights, strict=False)
        for k, v in ref.state_dict().items():
            if k not in weights:
                fwd[f"c{i}/buf/{k}"] = v.numpy()
        with torch.no_grad():
            fwd[f"c{i}/out1"] = ref(img, iters=1).numpy()
            fwd[f"c{i}/out3"] = ref(img, iters=3).numpy()
            fwd[f"c{i}/all3"] = ref(img, iters=3, return_all=True).numpy()

    ref = RefGlom(**BASE)
    ref.load_state_dict(weights, strict=True)
    with torch.no_grad():
        fwd["stateful/out"] = ref(img2, iters=2,
                                  levels=ref(img, iters=3)).numpy()

    # loss over the full trajectory reaches every parameter
    ref(img, iters=3, return_all=True).pow(2).mean().backward()
    grads = {"g/" + n: p.grad.numpy() for n, p in ref.named_parameters()}

    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN, "upstream_forward.npz"), **fwd)
    np.savez_compressed(os.path.join(GOLDEN, "upstream_grads.npz"), **grads)


if __name__ == "__main__":
    main(sys.argv[1])
