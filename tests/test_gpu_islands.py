"""Island-of-agreement analysis on the gfx950 HIP kernels: agreement
against an fp64 reference, labels against an independent union-find
oracle, hipGraph capture, determinism and dispatch."""

import numpy as np
import pytest
import torch

from conftest import SMALL, SMALL_BATCH, SMALL_ITERS
from _islands_util import (EXACT_CASES, agreement_atol, chain, channels,
                           min_margin, oracle_labels,
                           oracle_labels_of_agreement, oracle_sizes_count,
                           random_levels, ref_agreement64)

from glom_pytorch_amd import Glom, islands

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"

# (lead, H, W, L, D): D = 64 fills one lane-octet pass exactly, 72 and 520
# leave a ragged tail after 0 / 1 full 512-wide passes, 16x16x6x512 is the
# headline grid; 3x5 is non-square with W odd
RANDOM_SHAPES = [
    ((2,), 4, 4, 2, 64),
    ((1,), 3, 5, 3, 72),
    ((3, 2), 4, 4, 2, 520),
    ((1,), 16, 16, 6, 512),
]
SHAPE_IDS = ["4x4x2x64", "3x5x3x72", "3-2-4x4x2x520", "16x16x6x512"]

_cache = {}


def _random_case(i, connectivity):
    """Input, fp64 reference agreement and out-of-grid mask, built once."""
    key = (i, connectivity)
    if key not in _cache:
        lead, H, W, L, D = RANDOM_SHAPES[i]
        x = random_levels(lead, H, W, L, D, seed=10 + i)
        _cache[key] = (x, ref_agreement64(x, H, W, connectivity))
    return _cache[key]


def _np(t):
    return t.cpu().numpy()


def _out_of_grid(C, H, W):
    m = torch.zeros(C, H, W, dtype=torch.bool)
    m[0, :, W - 1] = True
    m[1, H - 1, :] = True
    if C == 4:
        m[2, H - 1, :] = True
        m[2, :, W - 1] = True
        m[3, H - 1, :] = True
        m[3, :, 0] = True
    return m


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("i", range(len(RANDOM_SHAPES)), ids=SHAPE_IDS)
def test_agreement_parity(i, connectivity):
    lead, H, W, L, D = RANDOM_SHAPES[i]
    x, ref = _random_case(i, connectivity)
    before = islands.native_calls()
    agr = islands.edge_agreement(x.to(DEV), grid=(H, W),
                                 connectivity=connectivity)
    assert islands.native_calls() == before + 1
    C = channels(connectivity)
    assert agr.dtype == torch.float32
    assert agr.shape == (*lead, L, C, H, W)
    err = (agr.cpu().double() - ref).abs().max().item()
    print(f"agreement max err {err:.3e} (atol {agreement_atol(D):.3e})")
    assert err <= agreement_atol(D)
    assert (agr.cpu()[..., _out_of_grid(C, H, W)] == 0).all()


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_labels_independent_oracle(case, connectivity):
    name, build, H, W, thr = case
    x = build()
    margin = min_margin(x, H, W, thr, connectivity)
    assert margin > 1e-3          # condition on the inputs (see CPU test)
    want = oracle_labels(x, H, W, thr, connectivity)
    before = islands.native_calls()
    labels = islands.island_labels(x.to(DEV), threshold=thr, grid=(H, W),
                                   connectivity=connectivity)
    assert islands.native_calls() > before
    assert labels.dtype == torch.int32 and labels.is_cuda
    assert np.array_equal(_np(labels), want)
    sizes, count = oracle_sizes_count(want)
    assert np.array_equal(_np(islands.island_sizes(labels)), sizes)
    assert np.array_equal(_np(islands.island_count(labels)), count)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_chain_32x32_converges(connectivity):
    """N = 1024 (the native maximum); the kept edges form one path of 1023
    hops per level, so a fixed small iteration count cannot label it."""
    H = W = 32
    x = chain(H, W, L=2)
    want = oracle_labels(x, H, W, 0.4, connectivity)
    assert want.max() == 0
    labels = islands.island_labels(x.to(DEV), threshold=0.4, grid=(H, W),
                                   connectivity=connectivity)
    assert np.array_equal(_np(labels), want)
    sizes, count = oracle_sizes_count(want)
    assert np.array_equal(_np(islands.island_sizes(labels)), sizes)
    assert np.array_equal(_np(islands.island_count(labels)), count)
    assert count.tolist() == [1, 1] and sizes[:, 0, 0].tolist() == [1024] * 2


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("i", range(len(RANDOM_SHAPES)), ids=SHAPE_IDS)
def test_labels_follow_returned_agreement(i, connectivity):
    lead, H, W, L, D = RANDOM_SHAPES[i]
    x, _ = _random_case(i, connectivity)
    xd = x.to(DEV)
    for thr in (0.0, 0.1):
        labels, agr = islands.island_labels(
            xd, threshold=thr, grid=(H, W), connectivity=connectivity,
            return_agreement=True)
        # exact: the decision is made in fp32 on the values returned
        want = oracle_labels_of_agreement(agr, thr)
        assert np.array_equal(_np(labels), want)
        before = islands.native_calls()
        direct = islands.labels_from_agreement(agr, thr,
                                               connectivity=connectivity)
        assert islands.native_calls() == before + 1
        assert torch.equal(direct, labels)
        sizes, count = oracle_sizes_count(want)
        assert np.array_equal(_np(islands.island_sizes(labels)), sizes)
        assert np.array_equal(_np(islands.island_count(labels)), count)


def test_model_level():
    model = Glom(**SMALL).to(DEV, torch.bfloat16)
    img = torch.randn(SMALL_BATCH, 3, SMALL["image_size"],
                      SMALL["image_size"], device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        slab = model(img, iters=SMALL_ITERS, return_all=True)
    side = model.num_patches_side
    labels = model.islands(slab, threshold=0.9, connectivity=8)
    assert labels.shape == (SMALL_ITERS + 1, SMALL_BATCH, SMALL["levels"],
                            side, side)
    own, agr = islands.island_labels(slab, threshold=0.9, grid=(side, side),
                                     connectivity=8, return_agreement=True)
    ref = ref_agreement64(slab, side, side, 8)
    err = (agr.cpu().double() - ref).abs().max().item()
    print(f"model slab agreement max err {err:.3e}")
    assert err <= agreement_atol(SMALL["dim"])
    assert torch.equal(labels, own)
    assert np.array_equal(_np(labels), oracle_labels_of_agreement(agr, 0.9))


def test_capturable_without_host_sync():
    lead, H, W, L, D = RANDOM_SHAPES[0]
    xs = [random_levels(lead, H, W, L, D, seed=s).to(DEV) for s in (20, 21)]
    eager = [islands.island_labels(x, threshold=0.1, grid=(H, W),
                                   return_agreement=True) for x in xs]
    static = xs[0].clone()
    islands.island_labels(static, threshold=0.1, grid=(H, W))   # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        labels, agr = islands.island_labels(static, threshold=0.1,
                                            grid=(H, W),
                                            return_agreement=True)
    for k in (1, 0):
        static.copy_(xs[k])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(labels, eager[k][0])
        assert torch.equal(agr, eager[k][1])
    assert not torch.equal(eager[0][0], eager[1][0])   # contents did differ


@pytest.mark.parametrize("connectivity", [4, 8])
def test_bitwise_deterministic(connectivity):
    lead, H, W, L, D = RANDOM_SHAPES[3]
    x, _ = _random_case(3, connectivity)
    xd = x.to(DEV)
    a = islands.island_labels(xd, threshold=0.05, grid=(H, W),
                              connectivity=connectivity,
                              return_agreement=True)
    b = islands.island_labels(xd, threshold=0.05, grid=(H, W),
                              connectivity=connectivity,
                              return_agreement=True)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_native_path_is_used_for_bf16_only():
    lead, H, W, L, D = RANDOM_SHAPES[0]
    x, ref = _random_case(0, 4)
    xd = x.to(DEV)
    n0 = islands.native_calls()
    nat, nat_agr = islands.island_labels(xd, threshold=0.1, grid=(H, W),
                                         return_agreement=True)
    n1 = islands.native_calls()
    assert n1 == n0 + 2                      # agreement + labelling kernels
    # fp32 levels take the torch implementation, on the GPU, and agree
    tor_agr = islands.edge_agreement(xd.float(), grid=(H, W))
    assert islands.native_calls() == n1
    assert tor_agr.is_cuda
    err = (tor_agr.cpu().double() - ref).abs().max().item()
    assert err <= agreement_atol(D)
    assert (nat_agr - tor_agr).abs().max().item() <= 2 * agreement_atol(D)
    tor = islands.island_labels(xd.float(), threshold=0.1, grid=(H, W))
    assert islands.native_calls() == n1 + 1  # fp32 agreement -> label kernel
    assert np.array_equal(_np(tor), oracle_labels_of_agreement(tor_agr, 0.1))
    # D not a multiple of 8 stays on the torch path too
    odd = random_levels((1,), 4, 4, 2, 20, seed=30).to(DEV)
    n2 = islands.native_calls()
    lab, agr = islands.island_labels(odd, threshold=0.1, grid=(4, 4),
                                     return_agreement=True)
    assert islands.native_calls() == n2 + 1  # only the fp32 labelling kernel
    assert np.array_equal(_np(lab), oracle_labels_of_agreement(agr, 0.1))
