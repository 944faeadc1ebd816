"""Every GEMM kernel family of run_gemm, bit-exact on integer probes.

Operands are integers in {-2..2} (bias in {-8..8}), so every product and
partial sum is an integer far below 2^24: the f32 accumulation is exact in
any order, with any split-K partition, and the one rounding left is the
final one to bf16. The kernel output must therefore equal the fp64 product
rounded once, bit for bit (tests/_bounds_util.py). A dropped k-tail, a
missing bias column, a swapped fragment or a wrong group offset (the G
problems are distinct) all change integers and cannot hide in a norm.

Shapes are the smallest per dispatch branch, (M, N, K, G); the subprocess
test at the end checks that each one reached the kernel it is listed under.
"""

import functools
import os
import subprocess
import sys

import pytest
import torch

from _bounds_util import assert_exact, int_probe
from test_gpu_tn_tr import GEMM_CASES as TN_CASES

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"

NT_CASES = [
    # generic predicated kernel: one partial tile; M, N, K tails; M = 129
    ((8, 8, 8, 1), "generic"),
    ((130, 72, 200, 2), "generic"),
    ((129, 136, 72, 1), "generic"),
    # 128^2 full-tile kernel: one K-step; 3 steps, 2 x 3 tiles, 3 groups
    ((128, 128, 64, 1), "nt_fast"),
    ((256, 384, 192, 3), "nt_fast"),
    # 128 x 256 ring kernel
    ((128, 1024, 64, 1), "nt4"),
    ((384, 1024, 192, 2), "nt4"),
    # persistent ring: the grid 4 * 4 * 6 = 96 is exactly the gate
    ((2048, 1024, 64, 6), "nt5p"),
    ((2048, 1024, 192, 6), "nt5p"),
    # 8-phase 256^2: the grid 2 * 8 * 16 = 256 is exactly the gate
    ((2048, 512, 2048, 16), "nt8p"),
    ((2048, 512, 2112, 16), "nt8p"),
]
NN_CASES = [
    ((128, 128, 8, 1), "nn_fast"),
    ((256, 128, 264, 2), "nn_fast"),
    ((72, 40, 24, 1), "generic"),
]
# default mode (1): split-K calls and K >= 4096 take gemm_tn_tr
TN_KERNELS = ["tn_fast", "tn_fast", "tn_tr", "tn_tr", "tn_fast", "generic"]


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(
        sum((i + 3) * int(k) for i, k in enumerate(key)))


@functools.lru_cache(maxsize=2)
def _nt_problem(M, N, K, G):
    g = _gen(M, N, K, G)
    A = int_probe((G, M, K), -2, 2, g)
    B = int_probe((G, N, K), -2, 2, g)
    bias = int_probe((G, N), -8, 8, g)
    ref = torch.matmul(A.double(), B.double().transpose(1, 2))
    return A, B, bias, ref


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", [c[0] for c in NT_CASES], ids=str)
def test_gemm_nt_exact(shape, bias):
    A, B, b, ref = _nt_problem(*shape)
    if bias:
        out = _ext().gemm_nt(A, B, b)
        assert_exact(out, ref + b.double()[:, None, :], "gemm_nt+bias")
    else:
        assert_exact(_ext().gemm_nt(A, B), ref, "gemm_nt")


@pytest.mark.parametrize("shape", [c[0] for c in NN_CASES], ids=str)
def test_gemm_nn_exact(shape):
    M, N, K, G = shape
    g = _gen(M, N, K, G, 1)
    A = int_probe((G, M, K), -2, 2, g)
    B = int_probe((G, K, N), -2, 2, g)
    assert_exact(_ext().gemm_nn(A, B), torch.matmul(A.double(), B.double()),
                 "gemm_nn")


@functools.lru_cache(maxsize=None)
def _tn_problem(M, N, K, G):
    g = _gen(M, N, K, G, 2)
    A = int_probe((G, K, M), -2, 2, g)
    B = int_probe((G, K, N), -2, 2, g)
    return A, B, torch.matmul(A.double().transpose(1, 2), B.double())


# (set_tn_tr_mode, split-K pipeline variant)
@pytest.mark.parametrize("mode,variant",
                         [(0, 1), (1, 1), (1, 2), (1, 3), (2, 1)])
@pytest.mark.parametrize("shape", TN_CASES, ids=str)
def test_gemm_tn_exact(shape, mode, variant):
    A, B, ref = _tn_problem(*shape)
    ext = _ext()
    mode0, var0 = ext.get_tn_tr_mode(), ext.get_tn_tr_variant()
    try:
        ext.set_tn_tr_mode(mode)
        ext.set_tn_tr_variant(variant)
        out = ext.gemm_tn(A, B)
        torch.cuda.synchronize()
    finally:
        ext.set_tn_tr_mode(mode0)
        ext.set_tn_tr_variant(var0)
    assert_exact(out, ref, "gemm_tn mode %d variant %d" % (mode, variant))


def test_shapes_reach_their_kernels():
    """Each shape above runs on the kernel it is listed under (the `kern=`
    field of the GLOM_DISPATCH_DEBUG line names the chosen launcher)."""
    code = (
        "import torch\n"
        "from glom_pytorch_amd.ops import _load_extension\n"
        "ext = _load_extension()\n"
        "z = lambda *s: torch.zeros(*s, device='cuda:0',"
        " dtype=torch.bfloat16)\n"
        "for (M, N, K, G) in %r:\n"
        "    ext.gemm_nt(z(G, M, K), z(G, N, K), z(G, N))\n"
        "for (M, N, K, G) in %r:\n"
        "    ext.gemm_nn(z(G, M, K), z(G, K, N))\n"
        "for (M, N, K, G) in %r:\n"
        "    ext.gemm_tn(z(G, K, M), z(G, K, N))\n"
        "torch.cuda.synchronize()\n"
        % ([c[0] for c in NT_CASES], [c[0] for c in NN_CASES], TN_CASES))
    env = dict(os.environ, GLOM_DISPATCH_DEBUG="1")
    for k in ("GLOM_TN_TR", "GLOM_NT8P", "GLOM_NT5P", "GLOM_NT5P_MING",
              "GLOM_NT8P_MINK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [ln for ln in r.stderr.splitlines() if "[dispatch]" in ln]
    want = ([(0, s, k) for s, k in NT_CASES]
            + [(1, s, k) for s, k in NN_CASES]
            + [(2, s, k) for s, k in zip(TN_CASES, TN_KERNELS)])
    assert len(lines) == len(want), lines
    for (layout, (M, N, K, G), kern), ln in zip(want, lines):
        assert "L%d M%d N%d K%d " % (layout, M, N, K) in ln, ln
        assert ln.rstrip().endswith("kern=" + kern), (kern, ln)
