"""Parse trees — what the islands are for. GLOM represents an image as a
part-whole tree: an island of agreeing patch columns at level l is a node,
and the island at level l+1 that lies over most of it is its parent. This
runs a model, builds the tree for every time step and image of the
`return_all=True` trajectory at once, and prints the nodes of one image. On
GPU the labels, the parent vote and the island mean vectors all come from
HIP kernels.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from glom_pytorch_amd import Glom, island_means
from glom_pytorch_amd.parse import tree_nodes

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

# labels, sizes, parents, overlap: int32 (T+1, B, L, side, side), stored at
# each island's root cell; means: fp32 (T+1, B, N, L, d), one row per island
tree = model.parse_tree(all_levels, threshold=0.9, connectivity=4)
side = model.num_patches_side
print(f"grid {side}x{side}; fields:",
      {k: tuple(v.shape) for k, v in tree._asdict().items()})

nodes = tree_nodes(tree, (iters, 0))          # final state of image 0
per_level = [sum(1 for n in nodes if n[0] == l) for l in range(model.levels)]
print("islands per level (bottom -> top):", per_level)
print("largest nodes: (level, root, size, parent, overlap)")
for node in sorted(nodes, key=lambda n: (-n[2], n[0], n[1]))[:8]:
    print("  ", node)

# what a node stands for: its island's mean vector
level, root = max(nodes, key=lambda n: n[2])[:2]
vec = tree.means[iters, 0, root, level]
print(f"node (level {level}, root {root}): |mean| = {vec.norm().item():.3f}")

# every column replaced by its island's mean, in the layout and dtype of a
# level state: this can seed another run of the model
pooled = island_means(all_levels[-1], tree.labels[-1], broadcast=True,
                      dtype=all_levels.dtype)
with torch.no_grad():
    again = model(img, iters=2, levels=pooled)
print("re-run from pooled state:", tuple(again.shape))
