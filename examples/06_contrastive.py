"""Contrastive regularisation of the top level — the contrastive half of the
reference README's open to-do ("contrastive / consistency regularization of
top-ish levels"; the consistency half is not built yet).
Two corruptions of the same images go through the model in one batch; the
embedding of a patch column at the top level should agree across the two
views and differ from the columns of other images. On GPU (bf16) the loss
and its gradient run on the HIP kernels without ever storing the
(B*N) x (B*N) logits. `DenoisingTrainer(contrast_weight=...)` adds the same
term to the denoising step.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from glom_pytorch_amd import Glom

use_gpu = torch.cuda.is_available()
dev = "cuda" if use_gpu else "cpu"
dtype = torch.bfloat16 if use_gpu else torch.float32
size, patch = (224, 14) if use_gpu else (32, 8)

torch.manual_seed(0)
model = Glom(dim=512 if use_gpu else 64, levels=6 if use_gpu else 3,
             image_size=size, patch_size=patch).to(dev, dtype)

B = 4
img = torch.randn(B, 3, size, size, device=dev, dtype=dtype)
views = torch.cat((img + torch.randn_like(img), img + torch.randn_like(img)))

levels = model(views, iters=model.levels)                   # (2B, N, L, d)
loss = model.contrastive_loss(levels[:B], levels[B:], level=-1,
                              temperature=0.1, negatives="other_images")
loss.backward()
grad = model.bottom_up.net[1].weight.grad
print(f"top-level contrastive loss {loss.item():.4f} "
      f"(grad norm {grad.float().norm().item():.3e})")
