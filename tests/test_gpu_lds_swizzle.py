"""Every kernel that stages through the swizzled [rows][64] LDS image,
bit-exact on structured integer probes (ops/csrc/lds_swizzle.h).

The swizzle only moves where bytes sit in LDS: writer and reader of an image
must agree on it, and then every MFMA sees the operands it saw before. The
probes make a disagreement visible. Operand element (row r, reduction index
k) is ((a*r + b*(k >> 3) + c*(k & 7) + 2*g) mod 11) - 5 with a, b, c coprime
to 11: two rows less than 11 apart differ, and so do any two of the eight
8-element k-granules of a 64-wide stage, so a row or granule delivered to
the wrong place changes integers. |value| <= 5 and K <= 4096: every partial
sum is an integer below 2^24, f32 accumulation is exact in any order, and
the kernel must return the CPU's exact product rounded once to bf16 (raw
f32 partials: the exact integers).

Each case is the smallest shape that run_gemm sends to the kernel (the
subprocess test at the end checks the `kern=` of each dispatch line); the
operands sit inside NaN-filled guard buffers, so a read outside them turns
up as NaN. gemm_nt_fast4 needs N >= 1024 through the dispatcher, nt5p and
nt8p their minimum grids: hence G = 24 and G = 256.

The fused consensus forward (softmax + AV inside gemm_nt_fast4) is not
integer valued. There the levels are in {-1, 0, 1}: the returned P must be
within the bf16 error budget of the fp64 softmax, and O must equal P @ V,
P as returned, exactly: with P in [2^-11, 2^-5] every product is a multiple
of 2^-19, a row's partial sums stay below 2^3, 22 bits, exact in f32.
"""

import functools
import os
import subprocess
import sys

import pytest
import torch

from _bounds_util import assert_exact, assert_within

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"
GUARD = 4096          # NaN elements on each side of an operand (16-byte mult.)

# (M, N, K, G), kernel
NT_CASES = [
    ((128, 128, 64, 1), "nt_fast"),
    ((128, 128, 192, 1), "nt_fast"),
    ((128, 1024, 192, 1), "nt4"),
    ((512, 1024, 256, 24), "nt5p"),     # grid 4 * 1 * 24 = 96: the gate
    ((256, 256, 2048, 256), "nt8p"),    # grid 1 * 1 * 256: the gate
]
NN_CASES = [((128, 128, 64, 1), "nn_fast"), ((128, 128, 192, 1), "nn_fast")]
# set_tn_tr_mode(0): the repack kernels; K >= 4096 splits 16 ways
TN_CASES = [((128, 128, 64, 1), "tn_fast"), ((128, 128, 192, 1), "tn_fast"),
            ((128, 128, 4096, 1), "tn_sk")]
GPERIOD = 16          # operands repeat with this period in g


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


def _pat(G, R, K, a, b, c):
    """(G, R, K) int64 on the CPU, see the module docstring."""
    g = torch.arange(G).view(G, 1, 1) % GPERIOD
    r = torch.arange(R).view(1, R, 1)
    k = torch.arange(K).view(1, 1, K)
    return (a * r + b * (k >> 3) + c * (k & 7) + 2 * g) % 11 - 5


def _wrap(t, G=None):
    """bf16 copy of the integer tensor `t` on the GPU, inside NaN guards;
    its leading (group) dimension repeated up to G."""
    g = t.shape[0]
    rep = (G or g) // g
    n = t.numel() * rep
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV,
                     dtype=torch.bfloat16)
    v = buf[GUARD:GUARD + n].view(rep, *t.shape)
    v.copy_(t.to(torch.bfloat16).to(DEV))
    return v.view(rep * g, *t.shape[1:])


@functools.lru_cache(maxsize=1)
def _problem(M, N, K, G):
    """A (g, M, K), B (g, N, K) integers and A B^T in fp64, g = min(G, 16)
    distinct groups (the operands are periodic in g)."""
    g = min(G, GPERIOD)
    A, B = _pat(g, M, K, 5, 3, 1), _pat(g, N, K, 7, 4, 2)
    ref = torch.matmul(A.double(), B.double().transpose(1, 2))
    return A, B, ref


@pytest.mark.parametrize("shape", [c[0] for c in NT_CASES], ids=str)
def test_nt_exact(shape):
    M, N, K, G = shape
    A, B, ref = _problem(*shape)
    out = _ext().gemm_nt(_wrap(A, G), _wrap(B, G))
    ref = ref.to(DEV).repeat(G // ref.shape[0], 1, 1)
    assert_exact(out, ref, "gemm_nt %s" % (shape,))


@pytest.mark.parametrize("shape", [c[0] for c in NN_CASES], ids=str)
def test_nn_exact(shape):
    A, B, ref = _problem(*shape)
    out = _ext().gemm_nn(_wrap(A), _wrap(B.transpose(1, 2).contiguous()))
    assert_exact(out, ref.to(DEV), "gemm_nn %s" % (shape,))


@pytest.mark.parametrize("shape", [c[0] for c in TN_CASES], ids=str)
def test_tn_exact(shape):
    A, B, ref = _problem(*shape)
    ext = _ext()
    mode0 = ext.get_tn_tr_mode()
    try:
        ext.set_tn_tr_mode(0)
        out = ext.gemm_tn(_wrap(A.transpose(1, 2).contiguous()),
                          _wrap(B.transpose(1, 2).contiguous()))
        torch.cuda.synchronize()
    finally:
        ext.set_tn_tr_mode(mode0)
    assert_exact(out, ref.to(DEV), "gemm_tn %s" % (shape,))


@pytest.mark.parametrize("K,sk", [(64, 1), (192, 2), (4096, 16)])
def test_nn_splitk_exact(K, sk):
    A, B, ref = _problem(128, 128, K, 1)
    ws = _ext().gemm_nn_splitk(_wrap(A),
                               _wrap(B.transpose(1, 2).contiguous()), sk)
    assert ws.shape == (sk, 1, 128, 128) and ws.dtype == torch.float32
    # integers below 2^24: each slice and their sum are exact in fp64
    assert torch.equal(ws.double().sum(0), ref.to(DEV))


def test_shapes_reach_their_kernels():
    code = (
        "import torch\n"
        "from glom_pytorch_amd.ops import _load_extension\n"
        "ext = _load_extension()\n"
        "z = lambda *s: torch.zeros(*s, device='cuda:0',"
        " dtype=torch.bfloat16)\n"
        "for (M, N, K, G) in %r:\n"
        "    ext.gemm_nt(z(G, M, K), z(G, N, K))\n"
        "for (M, N, K, G) in %r:\n"
        "    ext.gemm_nn(z(G, M, K), z(G, K, N))\n"
        "ext.set_tn_tr_mode(0)\n"
        "for (M, N, K, G) in %r:\n"
        "    ext.gemm_tn(z(G, K, M), z(G, K, N))\n"
        "torch.cuda.synchronize()\n"
        % tuple([c[0] for c in cases]
                for cases in (NT_CASES, NN_CASES, TN_CASES)))
    env = dict(os.environ, GLOM_DISPATCH_DEBUG="1")
    for k in ("GLOM_TN_TR", "GLOM_NT8P", "GLOM_NT5P", "GLOM_NT5P_MING",
              "GLOM_NT8P_MINK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [ln for ln in r.stderr.splitlines() if "[dispatch]" in ln]
    want = ([(0, s, k) for s, k in NT_CASES] + [(1, s, k) for s, k in NN_CASES]
            + [(2, s, k) for s, k in TN_CASES])
    assert len(lines) == len(want), lines
    for (layout, (M, N, K, G), kern), ln in zip(want, lines):
        assert "L%d M%d N%d K%d " % (layout, M, N, K) in ln, ln
        assert ln.rstrip().endswith("kern=" + kern), (kern, ln)


_TERNARY = torch.tensor([-1, 0, 1, 1, 0, -1, 1, -1, 0, 0, 1])


@pytest.mark.parametrize("d", [64, 512])
def test_fused_consensus_forward(d):
    """One problem (B = L = 1), N = 256: scores, softmax and the AV product
    all inside gemm_nt_fast4; V goes through the swizzled repack image, P is
    read from the padded epilogue rows."""
    N = 256
    j = torch.arange(N).view(N, 1)
    c = torch.arange(d).view(1, d)
    # all 256 rows distinct, and the 8-wide granules of a row distinct
    lv = _TERNARY[(7 * j + (13 + j // 11) * (c >> 3)
                   + (3 + j // 121) * (c & 7)) % 11]
    assert len(set(map(tuple, lv.tolist()))) == N
    out, probs, rnorm = _ext().consensus_fwd(
        _wrap(lv.view(1, N, 1, d)), False, None)
    torch.cuda.synchronize()
    out, probs = out.view(N, d).cpu(), probs.view(N, N).cpu()

    # P against the fp64 softmax. Error budget, relative: the bf16 score
    # (|score| <= 1, so exp moves by 2^-9), the bf16 exp, the row sum of
    # both (2 * 2^-9), the final bf16 rounding: 5 * 2^-9; 6 with the f32
    # steps and the fast exp.
    v = lv.double()
    sim = (v @ v.t()) * (1.0 / v.norm(dim=1)).view(1, N) * d ** -0.5
    assert float(sim.abs().max()) <= 1.0
    self_val = torch.tensor(-5e-4).to(torch.bfloat16).double()
    sim[torch.eye(N, dtype=torch.bool)] = self_val
    pref = sim.softmax(dim=1)
    worst = assert_within(probs, pref, 6 * 2.0 ** -9 * pref, "P d=%d" % d)
    print("consensus d=%d: worst P err / bound %.3f" % (d, worst))

    # O = P V exactly, P as the kernel rounded it
    assert float(probs.min()) >= 2.0 ** -11 and float(probs.max()) <= 2.0 ** -5
    assert_exact(out, probs.double() @ v, "O d=%d" % d)
