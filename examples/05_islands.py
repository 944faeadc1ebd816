"""Islands of agreement — the reason `return_all=True` exists (reference
README.md: "all the level data across iterations for clustering, from which
one can inspect for the theorized islands"). Runs the model, then labels
the connected groups of neighbouring patch columns whose embedding at a
level is nearly the same vector, for every time step and level at once. On
GPU the whole trajectory slab is analysed by the HIP island kernels.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from glom_pytorch_amd import Glom, edge_agreement, island_count, island_sizes

use_gpu = torch.cuda.is_available()
dev = "cuda" if use_gpu else "cpu"
dtype = torch.bfloat16 if use_gpu else torch.float32
size, patch = (224, 14) if use_gpu else (32, 8)

torch.manual_seed(0)
model = Glom(dim=512 if use_gpu else 64, levels=6 if use_gpu else 3,
             image_size=size, patch_size=patch).to(dev, dtype)

img = torch.randn(2, 3, size, size, device=dev, dtype=dtype)
iters = 2 * model.levels
with torch.no_grad():
    all_levels = model(img, iters=iters, return_all=True)   # (T+1,B,N,L,d)
print("trajectory:", tuple(all_levels.shape))

# (T+1, B, L, side, side) int32; a cell's label is the smallest linear
# index h*side+w of its island
labels = model.islands(all_levels, threshold=0.9, connectivity=4)
count = island_count(labels)                                # (T+1, B, L)
largest = island_sizes(labels).amax(dim=(-2, -1))           # (T+1, B, L)
side = model.num_patches_side
print(f"grid {side}x{side}: islands per level (bottom -> top), image 0")
for t in (0, 1, iters // 2, iters):
    print(f"  t={t:2d}  count {count[t, 0].tolist()}"
          f"  largest {largest[t, 0].tolist()}")

# the agreement the labels were decided on is available too
agr = edge_agreement(all_levels[-1], grid=(side, side))     # (B,L,2,H,W)
inner = agr[..., 0, :, :-1]
print("final right-neighbour agreement per level (mean):",
      [round(v, 3) for v in inner.mean(dim=(0, 2, 3)).tolist()])
