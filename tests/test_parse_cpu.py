"""Parse trees from islands: the torch specification of
``glom_pytorch_amd.parse`` against an independent plain-Python oracle, on
the CPU. Parents and overlap are exact; means are held to the derived bound
``(N + 1) * 2**-24 * max|levels|`` or, on exact inputs, to equality."""

import numpy as np
import pytest
import torch

from conftest import SMALL, SMALL_BATCH, SMALL_ITERS
from _parse_util import (EXACT_CASES, EXACT_IDS, LABEL_CASES, MEANS_CASES,
                         MEANS_IDS, as_tensor, check_broadcast,
                         check_means_fp32, check_parents, exact_case,
                         labels_of, levels_for, means_bound, means_case,
                         oracle_means64, oracle_parents, real_labels)

import glom_pytorch_amd
from glom_pytorch_amd import Glom, islands, parse


@pytest.mark.parametrize("name", list(LABEL_CASES))
def test_parents_oracle(name):
    labels = labels_of(name)
    n0 = parse.native_calls()
    parents, overlap = parse.island_parents(as_tensor(labels),
                                            return_overlap=True)
    assert parse.native_calls() == n0          # CPU: the torch path
    assert parents.shape == labels.shape
    check_parents(parents, overlap, name)
    only = parse.island_parents(as_tensor(labels))
    assert torch.equal(only, parents)


def test_parents_int64_labels():
    for name in ("rand-2-3x5xL2", "oor-3x5xL3", "tie"):
        labels = labels_of(name)
        parents, overlap = parse.island_parents(
            as_tensor(labels, dtype=torch.int64), return_overlap=True)
        check_parents(parents, overlap, name)


@pytest.mark.parametrize("name", ["tie", "tie-reversed"])
def test_tie_goes_to_smallest_parent(name):
    parents, overlap = parse.island_parents(as_tensor(labels_of(name)),
                                            return_overlap=True)
    assert parents[0].flatten()[5].item() == 3
    assert overlap[0].flatten()[5].item() == 2
    # cell 5 is a group key only; the other group of level 0 is keyed by 0
    assert parents[0].flatten()[0].item() == 1
    assert overlap[0].flatten()[0].item() == 12
    assert (parents[0].flatten()[[1, 2, 3, 4, 6]] == -1).all()
    assert (parents[1] == -1).all() and (overlap[1] == 0).all()


def test_single_level_has_no_parents():
    labels = as_tensor(labels_of("rand-2-4x4xL1"))
    parents, overlap = parse.island_parents(labels, return_overlap=True)
    assert (parents == -1).all() and (overlap == 0).all()


def test_extreme_group_sizes():
    parents, overlap = parse.island_parents(
        as_tensor(labels_of("extreme-32x32")), return_overlap=True)
    flat_p, flat_o = parents.flatten(2), overlap.flatten(2)
    # one 1024-cell group over singletons: every count is 1, smallest q wins
    assert flat_p[0, 0, 7].item() == 0 and flat_o[0, 0, 7].item() == 1
    assert (flat_o[0, 0].sum().item(), flat_o[1, 0].sum().item()) == (1, 1024)
    assert (flat_p[1, 0] == 7).all() and (flat_o[1, 0] == 1).all()


@pytest.mark.parametrize("i", range(len(MEANS_CASES)), ids=MEANS_IDS)
def test_means_fp32_bound(i):
    labels, x, ref, bound = means_case(i)
    out = parse.island_means(x, as_tensor(labels))
    check_means_fp32(out, labels, ref, bound)
    # fp32 levels of the same values follow the same specification
    out32 = parse.island_means(x.float(), as_tensor(labels,
                                                    dtype=torch.int64))
    check_means_fp32(out32, labels, ref, bound)


@pytest.mark.parametrize("i", range(len(MEANS_CASES)), ids=MEANS_IDS)
def test_means_bf16_rounds_once_and_broadcast(i):
    labels, x, ref, bound = means_case(i)
    lab = as_tensor(labels)
    out = parse.island_means(x, lab)
    out_bf = parse.island_means(x, lab, dtype=torch.bfloat16)
    assert out_bf.dtype == torch.bfloat16
    assert torch.equal(out_bf, out.to(torch.bfloat16))
    for dtype, root in ((torch.float32, out), (torch.bfloat16, out_bf)):
        out_b = parse.island_means(x, lab, broadcast=True, dtype=dtype)
        assert out_b.dtype == dtype and out_b.shape == x.shape
        check_broadcast(out_b, root, labels)
    out_b = parse.island_means(x, lab, broadcast=True)
    check_means_fp32(out_b, labels, oracle_means64(x, labels, True), bound,
                     broadcast=True)


@pytest.mark.parametrize("i", range(len(EXACT_CASES)), ids=EXACT_IDS)
def test_means_exact_inputs(i):
    labels, x, ref = exact_case(i)
    want = torch.from_numpy(ref).float()
    assert torch.equal(want.double(), torch.from_numpy(ref))  # fp32-exact
    lab = as_tensor(labels)
    assert torch.equal(parse.island_means(x, lab), want)
    assert torch.equal(parse.island_means(x, lab, dtype=torch.bfloat16),
                       want.to(torch.bfloat16))
    ref_b = torch.from_numpy(oracle_means64(x, labels, True)).float()
    assert torch.equal(parse.island_means(x, lab, broadcast=True), ref_b)


@pytest.mark.parametrize("which", ["planted", "chain"])
def test_real_labels(which):
    x, labels = real_labels(which)
    lab = labels.numpy()
    assert which != "chain" or lab.max() == 0      # one island per problem
    parents, overlap = parse.island_parents(labels, return_overlap=True)
    want_p, want_o = oracle_parents(lab)
    assert np.array_equal(parents.numpy(), want_p)
    assert np.array_equal(overlap.numpy(), want_o)
    out = parse.island_means(x, labels)
    check_means_fp32(out, lab, oracle_means64(x, lab), means_bound(x))


def test_parse_tree_and_nodes():
    x, labels = real_labels("planted")
    H = W = 6
    tree = parse.parse_tree(x, threshold=0.8, grid=(H, W))
    assert isinstance(tree, parse.ParseTree)
    assert tree._fields == ("labels", "sizes", "parents", "overlap", "means")
    assert torch.equal(tree.labels, labels)
    assert torch.equal(tree.sizes, islands.island_sizes(labels))
    want_p, want_o = oracle_parents(labels.numpy())
    assert np.array_equal(tree.parents.numpy(), want_p)
    assert np.array_equal(tree.overlap.numpy(), want_o)
    assert tree.means.dtype == torch.float32 and tree.means.shape == x.shape
    assert torch.equal(tree.means, parse.island_means(x, labels))

    nodes = parse.tree_nodes(tree, 1)
    assert nodes == parse.tree_nodes(tree, (1,))
    lab = labels[1].flatten(1).numpy()
    want = []
    for l in range(lab.shape[0]):
        for r in sorted(set(lab[l].tolist())):
            want.append((l, r, int((lab[l] == r).sum()),
                         int(want_p[1].reshape(3, -1)[l, r]),
                         int(want_o[1].reshape(3, -1)[l, r])))
    assert nodes == want
    assert all(type(v) is int for node in nodes for v in node)
    # every node below the top has a parent that is a node one level up
    keys = {(l, r) for l, r, *_ in nodes}
    for l, r, size, parent, ovl in nodes:
        if l < 2:
            assert (l + 1, parent) in keys and 1 <= ovl <= size
        else:
            assert parent == -1 and ovl == 0
    with pytest.raises(ValueError):
        parse.tree_nodes(tree, ())


def test_model_level():
    model = Glom(**SMALL)
    img = torch.randn(SMALL_BATCH, 3, SMALL["image_size"],
                      SMALL["image_size"])
    with torch.no_grad():
        slab = model(img, iters=SMALL_ITERS, return_all=True)
    side = model.num_patches_side
    tree = model.parse_tree(slab, threshold=0.9, connectivity=8)
    lead = (SMALL_ITERS + 1, SMALL_BATCH)
    grid_shape = (*lead, SMALL["levels"], side, side)
    for t in (tree.labels, tree.sizes, tree.parents, tree.overlap):
        assert t.shape == grid_shape and t.dtype == torch.int32
    assert tree.means.shape == slab.shape
    assert torch.equal(tree.labels,
                       model.islands(slab, threshold=0.9, connectivity=8))
    lab = tree.labels.numpy()
    want_p, want_o = oracle_parents(lab)
    assert np.array_equal(tree.parents.numpy(), want_p)
    assert np.array_equal(tree.overlap.numpy(), want_o)
    check_means_fp32(tree.means, lab, oracle_means64(slab, lab),
                     means_bound(slab))


def test_inputs_are_detached():
    labels = labels_of("rand-2-4x4xL2")
    x = levels_for(labels, 64).float().requires_grad_()
    out = parse.island_means(x, as_tensor(labels))
    assert not out.requires_grad


def test_argument_errors():
    lab = as_tensor(labels_of("rand-2-4x4xL2"))            # (2, 2, 4, 4)
    x = levels_for(labels_of("rand-2-4x4xL2"), 64)         # (2, 16, 2, 64)
    with pytest.raises(ValueError):
        parse.island_parents(lab[0, 0])                    # dim < 3
    with pytest.raises(ValueError):
        parse.island_parents(lab.float())                  # not integer
    with pytest.raises(ValueError):
        parse.island_means(x[0, 0], lab[0])                # levels dim < 3
    with pytest.raises(ValueError):
        parse.island_means(x[:, :15], lab)                 # H*W != N
    with pytest.raises(ValueError):
        parse.island_means(x, lab[:, :1])                  # L differs
    with pytest.raises(ValueError):
        parse.island_means(x, lab[:1])                     # lead mismatch
    with pytest.raises(ValueError):
        parse.island_means(x[0], lab)                      # lead rank
    with pytest.raises(ValueError):
        parse.island_means(x, lab, dtype=torch.float16)    # bad dtype
    with pytest.raises(ValueError):
        parse.island_means(x, lab, dtype=torch.float64)


def test_exports():
    for name in ("parse", "island_parents", "island_means", "parse_tree",
                 "ParseTree"):
        assert name in glom_pytorch_amd.__all__
        assert hasattr(glom_pytorch_amd, name)
    assert glom_pytorch_amd.parse_tree is parse.parse_tree
    assert parse.native_calls() >= 0
