"""Shared inputs and an independent oracle for the island tests.

The generators build level states whose values are exact in bf16, so the
margin between every neighbour cosine and the threshold a test uses is
known in advance. The oracle is a plain-Python union-find over the kept
in-grid edges with an fp64 cosine; it shares no code with
``glom_pytorch_amd.islands``.
"""

import numpy as np
import torch

# forward edge channels (dh, dw): right, down, down-right, down-left
EDGES = ((0, 1), (1, 0), (1, 1), (1, -1))


def channels(connectivity):
    return {4: 2, 8: 4}[connectivity]


def agreement_atol(D):
    """Worst-case fp32 accumulation error of one dot product and two norms
    over D exact bf16 x bf16 products, relative to |a||b|."""
    return 2 * D * 2.0 ** -24 + 1e-6


def _roundup(x, m):
    return (x + m - 1) // m * m


def _serpentine(H, W, by_columns=False):
    """Linear cell indices in boustrophedon visiting order."""
    order = []
    if by_columns:
        for w in range(W):
            hs = range(H) if w % 2 == 0 else range(H - 1, -1, -1)
            order += [h * W + w for h in hs]
    else:
        for h in range(H):
            ws = range(W) if h % 2 == 0 else range(W - 1, -1, -1)
            order += [h * W + w for w in ws]
    return order


def chain(H, W, L=1):
    """(N, L, D) bf16: the k-th cell of a serpentine path holds
    e_k + e_{k+1}. Path-adjacent cells have cosine exactly 0.5, every other
    pair exactly 0, so any threshold in (0, 0.5] keeps one island whose
    edges form a single path of N-1 hops. Odd levels snake by columns."""
    N = H * W
    D = _roundup(N + 1, 8)
    x = torch.zeros(N, L, D)
    for l in range(L):
        for k, cell in enumerate(_serpentine(H, W, by_columns=l % 2 == 1)):
            x[cell, l, k] = 1.0
            x[cell, l, k + 1] = 1.0
    return x.to(torch.bfloat16)


def pairs(H, W, L=1):
    """(N, L, D) bf16 one-hot prototypes, prototype id = linear index // 2:
    cosine 1 inside a pair, 0 otherwise. The last cell of a row and the
    first of the next can share a prototype without being neighbours."""
    N = H * W
    D = _roundup((N + 1) // 2, 8)
    x = torch.zeros(N, L, D)
    for i in range(N):
        x[i, :, i // 2] = 1.0
    return x.to(torch.bfloat16)


def planted(H, W, D=64, seed=0, L=2, sigma=0.02):
    """(N, L, D) bf16: rectangular blocks of cells share a random prototype
    plus N(0, sigma^2) noise; the block layout differs per level."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(H, W, L, D)
    for l in range(L):
        hc = sorted({0, H} | {int(v) for v in
                              torch.randint(1, H, (2,), generator=g)})
        wc = sorted({0, W} | {int(v) for v in
                              torch.randint(1, W, (2,), generator=g)})
        for h0, h1 in zip(hc[:-1], hc[1:]):
            for w0, w1 in zip(wc[:-1], wc[1:]):
                proto = torch.randn(D, generator=g)
                noise = torch.randn(h1 - h0, w1 - w0, D, generator=g)
                x[h0:h1, w0:w1, l] = proto + sigma * noise
    return x.reshape(H * W, L, D).to(torch.bfloat16)


def random_levels(lead, H, W, L, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*lead, H * W, L, D, generator=g).to(torch.bfloat16)


# --------------------------------------------------------------------- #
# oracle

def ref_agreement64(levels, H, W, connectivity):
    """fp64 cosine agreement (*lead, L, C, H, W) of the stored values;
    edges that leave the grid hold 0."""
    C = channels(connectivity)
    lead = tuple(levels.shape[:-3])
    L, D = levels.shape[-2:]
    x = levels.detach().cpu().double().reshape(-1, H, W, L, D)
    xn = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    out = torch.zeros(x.shape[0], L, C, H, W, dtype=torch.float64)
    for c in range(C):
        dh, dw = EDGES[c]
        for h in range(H):
            for w in range(W):
                h2, w2 = h + dh, w + dw
                if h2 < H and 0 <= w2 < W:
                    out[:, :, c, h, w] = (xn[:, h, w] * xn[:, h2, w2]).sum(-1)
    return out.reshape(*lead, L, C, H, W)


def _find(parent, i):
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def labels_from_kept(kept):
    """kept: bool array (*lead, L, C, H, W). Union-find over the in-grid
    kept edges; label = smallest linear index of the component.
    Returns int32 numpy (*lead, L, H, W)."""
    kept = np.asarray(kept)
    lead = kept.shape[:-3]
    C, H, W = kept.shape[-3:]
    flat = kept.reshape(-1, C, H, W)
    out = np.zeros((flat.shape[0], H, W), dtype=np.int32)
    for p in range(flat.shape[0]):
        parent = list(range(H * W))
        for c in range(C):
            dh, dw = EDGES[c]
            for h in range(H):
                for w in range(W):
                    h2, w2 = h + dh, w + dw
                    if not (h2 < H and 0 <= w2 < W):
                        continue          # structurally absent
                    if flat[p, c, h, w]:
                        a = _find(parent, h * W + w)
                        b = _find(parent, h2 * W + w2)
                        if a != b:
                            parent[max(a, b)] = min(a, b)
        out[p] = np.array([_find(parent, i) for i in range(H * W)],
                          dtype=np.int32).reshape(H, W)
    return out.reshape(*lead, H, W)


def oracle_labels(levels, H, W, threshold, connectivity):
    """Labels from the fp64 cosine of the stored values."""
    agr = ref_agreement64(levels, H, W, connectivity).numpy()
    return labels_from_kept(agr >= threshold)


def oracle_labels_of_agreement(agreement, threshold):
    """Labels decided on a returned fp32 agreement tensor, in fp32."""
    agr = agreement.detach().cpu().numpy().astype(np.float32)
    return labels_from_kept(agr >= np.float32(threshold))


def oracle_sizes_count(labels):
    """(sizes at root cells, island count) from an int label array."""
    labels = np.asarray(labels)
    H, W = labels.shape[-2:]
    flat = labels.reshape(-1, H * W)
    sizes = np.zeros_like(flat)
    for p in range(flat.shape[0]):
        for r in flat[p]:
            sizes[p, r] += 1
    count = (flat == np.arange(H * W)).sum(-1)
    return (sizes.reshape(labels.shape).astype(np.int32),
            count.reshape(labels.shape[:-2]).astype(np.int32))


def min_margin(levels, H, W, threshold, connectivity):
    """Smallest |agreement - threshold| over the in-grid edges (fp64)."""
    C = channels(connectivity)
    agr = ref_agreement64(levels, H, W, connectivity)
    m = float("inf")
    for c in range(C):
        dh, dw = EDGES[c]
        sub = agr[..., c, 0:H - dh, max(0, -dw):W - max(0, dw)]
        if sub.numel():
            m = min(m, float((sub - threshold).abs().min()))
    return m


# (name, builder, H, W, threshold): inputs with a known threshold margin
EXACT_CASES = [
    ("chain4x4", lambda: chain(4, 4, L=2), 4, 4, 0.4),
    ("chain8x8", lambda: chain(8, 8, L=2), 8, 8, 0.4),
    ("chain3x5", lambda: chain(3, 5, L=2), 3, 5, 0.4),
    ("pairs3x5", lambda: pairs(3, 5, L=2), 3, 5, 0.5),
    ("planted6x6", lambda: planted(6, 6, D=64, seed=0, L=2), 6, 6, 0.8),
]
