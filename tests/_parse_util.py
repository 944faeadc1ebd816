"""Shared inputs and an independent oracle for the parse-tree tests.

The oracle is plain Python over numpy arrays: dictionary counting for
parents and overlap, fp64 sums for the means. It shares no code with
``glom_pytorch_amd.parse``. Labels are built directly as integers, so the
parents tests depend on no float.
"""

import itertools

import numpy as np
import torch

from _islands_util import chain, planted

OUT_OF_RANGE = (-1, None, 2 ** 30)     # None stands for N itself


# --------------------------------------------------------------------- #
# oracle

def oracle_parents(labels):
    """labels: int array (*lead, L, H, W) -> (parents, overlap) int32."""
    labels = np.asarray(labels)
    L, H, W = labels.shape[-3:]
    N = H * W
    flat = labels.reshape(-1, L, N)
    parents = np.full(flat.shape, -1, dtype=np.int32)
    overlap = np.zeros(flat.shape, dtype=np.int32)
    for p in range(flat.shape[0]):
        for l in range(L - 1):
            votes = {}
            for n in range(N):
                r, q = int(flat[p, l, n]), int(flat[p, l + 1, n])
                if 0 <= r < N and 0 <= q < N:
                    votes.setdefault(r, {})
                    votes[r][q] = votes[r].get(q, 0) + 1
            for r, cnt in votes.items():
                top = max(cnt.values())
                parents[p, l, r] = min(q for q, c in cnt.items() if c == top)
                overlap[p, l, r] = top
    return parents.reshape(labels.shape), overlap.reshape(labels.shape)


def oracle_means64(levels, labels, broadcast=False):
    """levels: tensor (*lead, N, L, D); labels: int array (*lead, L, H, W).
    fp64 numpy (*lead, N, L, D): group means at the root rows (or at every
    member row), zero elsewhere."""
    x = levels.detach().cpu().double().numpy()
    N, L, D = x.shape[-3:]
    xf = x.reshape(-1, N, L, D)
    lab = np.asarray(labels).reshape(-1, L, N)
    out = np.zeros_like(xf)
    for p in range(xf.shape[0]):
        for l in range(L):
            groups = {}
            for n in range(N):
                r = int(lab[p, l, n])
                if 0 <= r < N:
                    groups.setdefault(r, []).append(n)
            for r, cells in groups.items():
                mean = xf[p, cells, l].sum(axis=0) / len(cells)
                if broadcast:
                    out[p, cells, l] = mean
                else:
                    out[p, r, l] = mean
    return out.reshape(x.shape)


def means_bound(levels):
    """(N + 1) * 2**-24 * A per (lead, level) problem, A the largest
    |levels| of the problem: a sequential fp32 sum of at most N terms plus
    one division. fp64 numpy, broadcastable against (*lead, N, L, D)."""
    x = levels.detach().cpu().double().abs()
    N = x.shape[-3]
    A = x.amax(dim=(-3, -1), keepdim=True)
    return ((N + 1) * 2.0 ** -24 * A).numpy()


def zero_rows(labels, broadcast=False):
    """bool (*lead, N, L): rows of the means that must be exactly zero."""
    labels = np.asarray(labels)
    L, H, W = labels.shape[-3:]
    N = H * W
    lab = labels.reshape(-1, L, N)
    zero = np.ones((lab.shape[0], N, L), dtype=bool)
    for p in range(lab.shape[0]):
        for l in range(L):
            for n in range(N):
                r = int(lab[p, l, n])
                if 0 <= r < N:
                    zero[p, n if broadcast else r, l] = False
    return zero.reshape(*labels.shape[:-3], N, L)


# --------------------------------------------------------------------- #
# label generators: int64 numpy (*lead, L, H, W)

def random_labels(lead, H, W, L, seed=0):
    """Non-canonical labels: every (lead, level) problem draws about N/4
    keys anywhere in [0, N) and gives each cell one of them."""
    rng = np.random.default_rng(seed)
    N = H * W
    P = int(np.prod(lead, dtype=np.int64))
    out = np.zeros((P, L, N), dtype=np.int64)
    for p in range(P):
        for l in range(L):
            keys = rng.choice(N, size=max(1, N // 4), replace=False)
            out[p, l] = rng.choice(keys, size=N)
    return out.reshape(*lead, L, H, W)


def tie_labels(reverse):
    """4x4, L=2. Group 5 of level 0 is the cells {0,1,2,3} (cell 5 itself
    belongs to group 0); one level up it is split 2/2 between q=9 and q=3,
    in either cell order."""
    lab = np.zeros((2, 16), dtype=np.int64)
    lab[0, :4] = 5
    lab[1, :] = 1
    lab[1, :4] = [3, 3, 9, 9] if reverse else [9, 9, 3, 3]
    return lab.reshape(2, 4, 4)


def extreme_labels():
    """(2, 2, 32, 32): one group of 1024 cells under 1024 singleton groups
    (a permutation, so not canonical), and the other way round."""
    rng = np.random.default_rng(5)
    one = np.full(1024, 7, dtype=np.int64)
    lab = np.stack([np.stack([one, rng.permutation(1024)]),
                    np.stack([rng.permutation(1024), one])])
    return lab.reshape(2, 2, 32, 32)


def out_of_range_labels(lead, H, W, L, seed=0):
    """random_labels with about a third of the cells replaced by -1, N and
    2**30."""
    rng = np.random.default_rng(seed + 100)
    lab = random_labels(lead, H, W, L, seed)
    N = H * W
    bad = np.array([N if v is None else v for v in OUT_OF_RANGE])
    hit = rng.random(lab.shape) < 1 / 3
    lab[hit] = rng.choice(bad, size=int(hit.sum()))
    return lab


def pow2_labels(lead, H, W, L, seed=0):
    """Every group size is a power of two: a random permutation of the
    cells is cut into runs of N/2, N/4, ..., 1, 1 cells (N a power of two)
    and each run is keyed by one of its own cells."""
    rng = np.random.default_rng(seed)
    N = H * W
    assert N & (N - 1) == 0
    P = int(np.prod(lead, dtype=np.int64))
    out = np.zeros((P, L, N), dtype=np.int64)
    for p in range(P):
        for l in range(L):
            perm = rng.permutation(N)
            sizes, s = [], N // 2
            while s >= 1:
                sizes.append(s)
                s //= 2
            sizes.append(1)                  # N/2 + ... + 1 + 1 == N
            start = 0
            for s in sizes:
                run = perm[start:start + s]
                out[p, l, run] = rng.choice(run)
                start += s
            assert start == N
            got = np.bincount(out[p, l], minlength=N)
            assert all(s & (s - 1) == 0 for s in got)
    return out.reshape(*lead, L, H, W)


GRIDS = [(1, 1), (3, 5), (4, 4), (16, 16), (32, 32)]
LEVELS = [1, 2, 6]
LEADS = [(), (2,), (3, 2)]


def _name(lead, H, W, L):
    return "-".join(map(str, lead)) + f"{'-' if lead else ''}{H}x{W}xL{L}"


# name -> builder of int64 labels (*lead, L, H, W)
LABEL_CASES = {}
for _i, ((_H, _W), _L, _lead) in enumerate(
        itertools.product(GRIDS, LEVELS, LEADS)):
    LABEL_CASES["rand-" + _name(_lead, _H, _W, _L)] = (
        lambda a=(_lead, _H, _W, _L), s=_i: random_labels(*a, seed=s))
LABEL_CASES["tie"] = lambda: tie_labels(False)
LABEL_CASES["tie-reversed"] = lambda: tie_labels(True)
LABEL_CASES["extreme-32x32"] = extreme_labels
LABEL_CASES["oor-3x5xL3"] = lambda: out_of_range_labels((), 3, 5, 3, seed=1)
LABEL_CASES["oor-2-16x16xL3"] = (
    lambda: out_of_range_labels((2,), 16, 16, 3, seed=2))
LABEL_CASES["oor-32x32xL2"] = (
    lambda: out_of_range_labels((), 32, 32, 2, seed=3))

# (label case, D): D = 64 leaves 56 of a wave's lanes without data, 72 is
# ragged, 520 is one full 512-wide pass plus a tail, 512 one pass exactly
MEANS_CASES = [
    ("rand-1x1xL1", 64),
    ("rand-2-1x1xL6", 520),
    ("rand-2-3x5xL2", 72),
    ("rand-3-2-3x5xL1", 64),
    ("rand-4x4xL2", 512),
    ("rand-3-2-4x4xL6", 520),
    ("rand-16x16xL6", 512),
    ("rand-2-16x16xL2", 72),
    ("rand-2-32x32xL2", 64),
    ("rand-32x32xL6", 72),
    ("tie", 64),
    ("extreme-32x32", 64),
    ("extreme-32x32", 520),
    ("oor-3x5xL3", 72),
    ("oor-2-16x16xL3", 512),
    ("oor-32x32xL2", 64),
]
MEANS_IDS = [f"{n}-D{d}" for n, d in MEANS_CASES]

# (lead, H, W, L, D) of the exact-input cases (N a power of two)
EXACT_CASES = [
    ((), 1, 1, 2, 64),
    ((2,), 4, 4, 2, 72),
    ((), 16, 16, 6, 512),
    ((3, 2), 4, 4, 3, 520),
    ((), 32, 32, 2, 64),
]
EXACT_IDS = [_name(*c[:4]) + f"-D{c[4]}" for c in EXACT_CASES]

_cache = {}


def labels_of(name):
    """int64 numpy labels of a LABEL_CASES entry, built once."""
    key = ("labels", name)
    if key not in _cache:
        _cache[key] = LABEL_CASES[name]()
        _cache[key].setflags(write=False)
    return _cache[key]


def parents_of(name):
    """Oracle (parents, overlap) of a LABEL_CASES entry, computed once."""
    key = ("parents", name)
    if key not in _cache:
        _cache[key] = oracle_parents(labels_of(name))
    return _cache[key]


def levels_for(labels, D, seed=0):
    """bf16 N(0,1) level states (*lead, N, L, D) that fit labels."""
    L, H, W = labels.shape[-3:]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*labels.shape[:-3], H * W, L, D,
                       generator=g).to(torch.bfloat16)


def means_case(i):
    """(labels, levels, fp64 root means, bound) of MEANS_CASES[i], once."""
    key = ("means", i)
    if key not in _cache:
        name, D = MEANS_CASES[i]
        labels = labels_of(name)
        x = levels_for(labels, D, seed=40 + i)
        _cache[key] = (labels, x, oracle_means64(x, labels), means_bound(x))
    return _cache[key]


def exact_case(i):
    """(labels, levels, fp64 root means) of EXACT_CASES[i]: integer level
    values with |v| <= 8 and power-of-two group sizes. Every partial sum
    is an integer with |s| <= 8 * 1024 and the mean is that integer over
    2**k, so both are exact in fp32 in any order; the bf16 result is the
    one rounding of that exact value."""
    key = ("exact", i)
    if key not in _cache:
        lead, H, W, L, D = EXACT_CASES[i]
        labels = pow2_labels(lead, H, W, L, seed=60 + i)
        g = torch.Generator().manual_seed(70 + i)
        x = torch.randint(-8, 9, (*lead, H * W, L, D),
                          generator=g).to(torch.bfloat16)
        _cache[key] = (labels, x, oracle_means64(x, labels))
    return _cache[key]


def real_labels(which, device="cpu"):
    """(levels, int32 labels) from island_labels on planted / chain level
    states of tests/_islands_util.py; levels (2, N, L, D) bf16."""
    from glom_pytorch_amd import islands
    if which == "planted":
        H, W, thr = 6, 6, 0.8
        x = torch.stack([planted(H, W, D=64, seed=s, L=3) for s in (0, 1)])
    else:
        H, W, thr = 3, 5, 0.4
        x = torch.stack([chain(H, W, L=2), chain(H, W, L=2).flip(0)])
    x = x.to(device)
    labels = islands.island_labels(x, threshold=thr, grid=(H, W))
    return x, labels


# --------------------------------------------------------------------- #
# checks shared by the CPU and the GPU tests

def as_tensor(labels, device="cpu", dtype=torch.int32):
    return torch.tensor(np.asarray(labels), dtype=dtype, device=device)


def check_parents(parents, overlap, name):
    want_p, want_o = parents_of(name)
    assert parents.dtype == torch.int32 and overlap.dtype == torch.int32
    assert np.array_equal(parents.cpu().numpy(), want_p)
    assert np.array_equal(overlap.cpu().numpy(), want_o)


def check_means_fp32(out, labels, ref64, bound, broadcast=False):
    """|out - ref64| <= bound everywhere; rows that must be zero are."""
    assert out.dtype == torch.float32 and tuple(out.shape) == ref64.shape
    got = out.cpu().double().numpy()
    err = np.abs(got - ref64)
    print(f"means max err {err.max():.3e}, smallest bound {bound.min():.3e}")
    assert (err <= bound).all()
    assert (got[zero_rows(labels, broadcast)] == 0).all()


def check_broadcast(out_b, out_root, labels):
    """out_b[n, l] == out_root[labels[l, n], l] bitwise for in-range labels
    and zero rows elsewhere."""
    N, L, D = out_root.shape[-3:]
    b = out_b.cpu().reshape(-1, N, L, D)
    root = out_root.cpu().reshape(-1, N, L, D)
    lab = torch.tensor(np.asarray(labels).reshape(-1, L, N))
    ok = (lab >= 0) & (lab < N)
    at = lab.clamp(0, N - 1).permute(0, 2, 1)                 # (P, N, L)
    want = root.gather(1, at.unsqueeze(-1).expand(-1, -1, -1, D))
    want = torch.where(ok.permute(0, 2, 1).unsqueeze(-1), want,
                       torch.zeros_like(want))
    assert torch.equal(b, want)
