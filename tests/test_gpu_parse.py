"""Parse trees on the gfx950 HIP kernels: parents and overlap against an
independent dictionary-counting oracle (exact), island means against fp64
within ``(N + 1) * 2**-24 * max|levels|`` and bit for bit on exact inputs,
hipGraph capture, determinism and dispatch."""

import numpy as np
import pytest
import torch

from conftest import SMALL, SMALL_BATCH, SMALL_ITERS
from _islands_util import planted
from _parse_util import (EXACT_CASES, EXACT_IDS, LABEL_CASES, MEANS_CASES,
                         MEANS_IDS, as_tensor, check_broadcast,
                         check_means_fp32, check_parents, exact_case,
                         labels_of, levels_for, means_bound, means_case,
                         oracle_means64, oracle_parents, real_labels)

from glom_pytorch_amd import Glom, islands, parse

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"


@pytest.mark.parametrize("name", list(LABEL_CASES))
def test_parents_oracle(name):
    labels = labels_of(name)
    before = parse.native_calls()
    parents, overlap = parse.island_parents(as_tensor(labels, DEV),
                                            return_overlap=True)
    assert parse.native_calls() == before + 1
    assert parents.is_cuda and parents.shape == labels.shape
    check_parents(parents, overlap, name)


@pytest.mark.parametrize("name", ["tie", "tie-reversed"])
def test_tie_goes_to_smallest_parent(name):
    before = parse.native_calls()
    parents, overlap = parse.island_parents(as_tensor(labels_of(name), DEV),
                                            return_overlap=True)
    assert parse.native_calls() == before + 1
    assert parents[0].flatten()[5].item() == 3
    assert overlap[0].flatten()[5].item() == 2
    assert (parents[1] == -1).all() and (overlap[1] == 0).all()


@pytest.mark.parametrize("i", range(len(MEANS_CASES)), ids=MEANS_IDS)
def test_means_fp32_bf16_broadcast(i):
    labels, x, ref, bound = means_case(i)
    xd, lab = x.to(DEV), as_tensor(labels, DEV)
    before = parse.native_calls()
    out = parse.island_means(xd, lab)
    out_bf = parse.island_means(xd, lab, dtype=torch.bfloat16)
    out_b = parse.island_means(xd, lab, broadcast=True)
    out_b_bf = parse.island_means(xd, lab, broadcast=True,
                                  dtype=torch.bfloat16)
    assert parse.native_calls() == before + 4
    assert out.is_cuda and out.shape == x.shape
    check_means_fp32(out, labels, ref, bound)
    # the kernel rounds once from the same fp32 value
    assert out_bf.dtype == torch.bfloat16
    assert torch.equal(out_bf, out.to(torch.bfloat16))
    check_broadcast(out_b, out, labels)
    check_broadcast(out_b_bf, out_bf, labels)


@pytest.mark.parametrize("i", range(len(EXACT_CASES)), ids=EXACT_IDS)
def test_means_exact_inputs(i):
    labels, x, ref = exact_case(i)
    want = torch.from_numpy(ref).float()
    xd, lab = x.to(DEV), as_tensor(labels, DEV)
    before = parse.native_calls()
    out = parse.island_means(xd, lab)
    out_bf = parse.island_means(xd, lab, dtype=torch.bfloat16)
    out_b = parse.island_means(xd, lab, broadcast=True)
    assert parse.native_calls() == before + 3
    assert torch.equal(out.cpu(), want)
    assert torch.equal(out_bf.cpu(), want.to(torch.bfloat16))
    ref_b = torch.from_numpy(oracle_means64(x, labels, True)).float()
    assert torch.equal(out_b.cpu(), ref_b)


def test_unaligned_levels_are_cloned():
    labels, x, ref, bound = means_case(4)              # 4x4, L=2, D=512
    buf = torch.empty(x.numel() + 8, dtype=torch.bfloat16, device=DEV)
    view = buf[4:4 + x.numel()].view(x.shape)          # 8-byte aligned only
    view.copy_(x)
    assert view.data_ptr() % 16 == 8
    before = parse.native_calls()
    out = parse.island_means(view, as_tensor(labels, DEV))
    assert parse.native_calls() == before + 1
    check_means_fp32(out, labels, ref, bound)


@pytest.mark.parametrize("which", ["planted", "chain"])
def test_real_labels(which):
    x, labels = real_labels(which, DEV)
    assert labels.is_cuda and labels.dtype == torch.int32
    lab = labels.cpu().numpy()
    before = parse.native_calls()
    parents, overlap = parse.island_parents(labels, return_overlap=True)
    out = parse.island_means(x, labels)
    assert parse.native_calls() == before + 2
    want_p, want_o = oracle_parents(lab)
    assert np.array_equal(parents.cpu().numpy(), want_p)
    assert np.array_equal(overlap.cpu().numpy(), want_o)
    check_means_fp32(out, lab, oracle_means64(x, lab), means_bound(x))


def test_bitwise_deterministic():
    labels, x, _, _ = means_case(MEANS_IDS.index("rand-16x16xL6-D512"))
    xd, lab = x.to(DEV), as_tensor(labels, DEV)
    before = parse.native_calls()
    for kw in (dict(), dict(broadcast=True), dict(dtype=torch.bfloat16)):
        a = parse.island_means(xd, lab, **kw)
        b = parse.island_means(xd, lab, **kw)
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32
                                  else torch.int16),
                           b.view(torch.int32 if b.dtype == torch.float32
                                  else torch.int16))
    pa = parse.island_parents(lab, return_overlap=True)
    pb = parse.island_parents(lab, return_overlap=True)
    assert parse.native_calls() == before + 8
    assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1])


def test_capturable_without_host_sync():
    H = W = 6
    xs = [torch.stack([planted(H, W, D=64, seed=s, L=3),
                       planted(H, W, D=64, seed=s + 1, L=3)]).to(DEV)
          for s in (20, 30)]
    eager = [parse.parse_tree(x, threshold=0.8, grid=(H, W)) for x in xs]
    static = xs[0].clone()
    parse.parse_tree(static, threshold=0.8, grid=(H, W))       # warm-up
    torch.cuda.synchronize()
    before = parse.native_calls()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tree = parse.parse_tree(static, threshold=0.8, grid=(H, W))
    assert parse.native_calls() == before + 2
    for k in (1, 0):
        static.copy_(xs[k])
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(tree, eager[k]):
            assert torch.equal(got, want)
    assert not torch.equal(eager[0].labels, eager[1].labels)  # did differ


def test_torch_path_on_gpu_for_everything_else():
    labels, x, ref, bound = means_case(2)              # (2,) 3x5, L=2, D=72
    name = MEANS_CASES[2][0]
    xd, lab = x.to(DEV), as_tensor(labels, DEV)
    n0 = parse.native_calls()
    # fp32 levels
    out = parse.island_means(xd.float(), lab)
    assert out.is_cuda
    check_means_fp32(out, labels, ref, bound)
    # int64 labels, both functions
    lab64 = as_tensor(labels, DEV, torch.int64)
    out = parse.island_means(xd, lab64, broadcast=True)
    check_means_fp32(out, labels, oracle_means64(x, labels, True), bound,
                     broadcast=True)
    parents, overlap = parse.island_parents(lab64, return_overlap=True)
    assert parents.is_cuda
    check_parents(parents, overlap, name)
    # D not a multiple of 8
    x20 = levels_for(labels, 20, seed=3)
    out = parse.island_means(x20.to(DEV), lab)
    check_means_fp32(out, labels, oracle_means64(x20, labels),
                     means_bound(x20))
    assert parse.native_calls() == n0                  # none of them native
    parse.island_means(xd, lab)
    assert parse.native_calls() == n0 + 1


def test_model_level():
    model = Glom(**SMALL).to(DEV, torch.bfloat16)
    img = torch.randn(SMALL_BATCH, 3, SMALL["image_size"],
                      SMALL["image_size"], device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        slab = model(img, iters=SMALL_ITERS, return_all=True)
    side = model.num_patches_side
    before = parse.native_calls()
    tree = model.parse_tree(slab, threshold=0.9, connectivity=8)
    assert parse.native_calls() == before + 2
    lead = (SMALL_ITERS + 1, SMALL_BATCH)
    for t in (tree.labels, tree.sizes, tree.parents, tree.overlap):
        assert t.shape == (*lead, SMALL["levels"], side, side)
        assert t.dtype == torch.int32 and t.is_cuda
    assert tree.means.shape == slab.shape
    assert tree.means.dtype == torch.float32
    assert torch.equal(tree.labels,
                       model.islands(slab, threshold=0.9, connectivity=8))
    assert torch.equal(tree.sizes, islands.island_sizes(tree.labels))
    lab = tree.labels.cpu().numpy()
    want_p, want_o = oracle_parents(lab)
    assert np.array_equal(tree.parents.cpu().numpy(), want_p)
    assert np.array_equal(tree.overlap.cpu().numpy(), want_o)
    check_means_fp32(tree.means, lab, oracle_means64(slab, lab),
                     means_bound(slab))
    nodes = parse.tree_nodes(tree, (SMALL_ITERS, 0))
    assert sum(n[2] for n in nodes) == SMALL["levels"] * side * side
