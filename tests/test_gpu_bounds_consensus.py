"""Consensus attention, stage by stage, against fp64 computed from the
kernel's own previous-stage output (ext.consensus_fwd returns out, probs,
rnorm; ext.consensus_bwd the gradient). u = 2^-8 is the bf16 roundoff.

rnorm = 1 / max(||x||, 1e-12) (F.normalize's formula): d exact squares
summed in f32 in any order, one sqrt, one divide: relative (d+4) * 2^-24.

probs. The score s_ij = (x_i . x_j) * d^-0.5 * rnorm_j is computed in f32
and rounded to bf16 before the exponential (the fused epilogue stages it in
LDS as bf16, the unfused path stores it), so the exponent carries the
absolute error
    E_ij = u * |s_ij| + (d+3) * 2^-23 * A_ij,   A = (|x_i| . |x_j|) * ...
(bf16 rounding plus any-order f32 accumulation; 0 on the self-masked
diagonal, which is the constant bf16(-5e-4)). p_j = e^{s_j} / sum_k e^{s_k}
is then off by at most a factor e^{E_j + max_k E_k}: its own exponent and
the denominator, a weighted mean of the e^{E_k}. The kernels then round the
unnormalised exponential to bf16 (the f32 sum uses the unrounded values) and
the normalised value to bf16: two more factors (1 + u). The N % 8 != 0
softmax keeps the exponential in f32 and rounds only the result: one factor.
The f32 work left (__expf with |argument| <= 32, the N-term sum, 1/sum, one
multiply, the f32 d^-0.5) gets a factor 1 + (N + 64) * 2^-23. So
    |p - ref| <= ref * (e^{E_j + Emax_i} (1+u)^r (1 + (N+64) 2^-23) - 1),
r = 2, or 1 when N % 8 != 0. Non-local-masked entries are exactly 0. Every
reference probability is asserted to stay above 2^-20, so no exponential
comes near the bf16 subnormals. A row sums to 1 within N * u (each term is
within 2u + u^2 of its share of an exact partition of 1).

out = probs @ levels: gemm_tol with K = N against the stored probs.

Backward, from the stored probs and rnorm (x, g = levels, dOut):
    dP = g x^T                         -> bf16   (1)
    dS = d^-0.5 P (dP - rowsum(P dP))  -> bf16   (2)  masked -> 0
    dSr = dS * rnorm_j (from the unrounded dS)  -> bf16   (2)
    dv = P^T g                         -> bf16   (1)
    dq = dSr x                         -> bf16   (3)
    dkhat = dS^T x                     -> bf16   (3)
    dLevels = r (dkhat - x r^2 (dkhat . x)) + dv + dq   -> bf16   (4)
(for a row clamped at eps, k = x / eps and the projection term is absent:
the eager formula's derivative). The longest path has 4 bf16 roundings. To
first order each rounding perturbs its value by at most u times the value,
and that perturbation reaches the result through the same linear chain; run
on absolute values (every subtraction an addition) the chain bounds both, so
    |dLevels - ref| <= (4 + 1) * u * chain(|.|),
the + 1 covering the f32 accumulations ((N+3) * 2^-23 << u) and second-order
terms.

Inputs are 0.5 * randn, with one all-zero row (rnorm clamps at 1e12) and
one row of norm 1e-3.
"""

import os
import subprocess
import sys

import pytest
import torch

from _bounds_util import U, assert_within, gemm_tol

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"
BF = torch.bfloat16
B, L = 2, 2
EPS32 = 2.0 ** -23


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


def _radius_mask(side, radius):
    hh, ww = torch.meshgrid(torch.arange(side), torch.arange(side),
                            indexing="ij")
    c = torch.stack((hh, ww)).float().reshape(2, -1).t()
    return (torch.cdist(c, c) > float(radius)).to(DEV).contiguous()


def _inputs(N, d):
    g = torch.Generator(device=DEV).manual_seed(1000 * N + d)
    lv = 0.5 * torch.randn(B, N, L, d, device=DEV, generator=g)
    lv[0, 1, 0] = 0
    v = torch.randn(d, device=DEV, generator=g)
    lv[1, 2, 1] = v / v.norm() * 1e-3
    dOut = torch.randn(B, N, L, d, device=DEV, generator=g)
    return lv.to(BF), dOut.to(BF)


def check_consensus(N, d, attend_self, mask):
    ext = _ext()
    levels, dOut = _inputs(N, d)
    out, probs, rnorm = ext.consensus_fwd(levels, attend_self, mask)
    dLev = ext.consensus_bwd(dOut, levels, probs, rnorm, attend_self, mask)
    tag = "N%d d%d self%d mask%d " % (N, d, attend_self, mask is not None)
    alpha = float(d) ** -0.5
    x = levels.double().permute(0, 2, 1, 3)                  # (B, L, N, d)
    g = dOut.double().permute(0, 2, 1, 3)
    ax, ag = x.abs(), g.abs()
    eye = torch.eye(N, device=DEV, dtype=torch.bool)
    dead = torch.zeros(N, N, device=DEV, dtype=torch.bool)   # exact zeros
    if mask is not None:
        dead = dead | mask
    const = dead if attend_self else dead | eye              # not from x
    fig = {}

    # ---- rnorm
    norm = x.norm(dim=-1)
    rn_ref = 1.0 / norm.clamp_min(1e-12)
    assert float(norm[0, 0, 1]) == 0 and abs(float(norm[1, 1, 2]) - 1e-3) < 1e-4
    fig["rnorm"] = assert_within(rnorm, rn_ref, (d + 4) * 2.0 ** -24 * rn_ref,
                                 tag + "rnorm")
    r = rnorm.double()

    # ---- probs, from the kernel's rnorm
    s = torch.matmul(x, x.transpose(-1, -2)) * alpha * r[:, :, None, :]
    A = torch.matmul(ax, ax.transpose(-1, -2)) * alpha * r[:, :, None, :]
    E = U * s.abs() + (d + 3) * EPS32 * A
    if not attend_self:
        s = s.masked_fill(eye, torch.tensor(-5e-4).to(BF).item())
    s = s.masked_fill(dead, float("-inf"))
    E = E.masked_fill(const, 0.0)
    assert float(s.masked_fill(dead, 0.0).abs().max()) <= 16   # |arg| <= 32
    p_ref = torch.softmax(s, dim=-1)
    assert float(p_ref.masked_fill(dead, 1.0).min()) > 2.0 ** -20
    assert float(p_ref.masked_fill(~dead, 0.0).max()) == 0
    nround = 2 if N % 8 == 0 else 1
    rel = (torch.exp(E + E.amax(-1, keepdim=True)) * (1 + U) ** nround
           * (1 + (N + 64) * EPS32) - 1)
    fig["probs"] = assert_within(probs, p_ref, rel * p_ref, tag + "probs")
    P = probs.double()
    assert float(P.masked_fill(~dead, 0.0).abs().max()) == 0
    rowsum = P.sum(-1)
    fig["rowsum"] = assert_within(rowsum, torch.ones_like(rowsum), N * U,
                                  tag + "row sums")

    # ---- out, from the kernel's probs
    o_ref = torch.matmul(P, x).permute(0, 2, 1, 3)
    o_abs = torch.matmul(P, ax).permute(0, 2, 1, 3)
    fig["out"] = assert_within(out, o_ref, gemm_tol(o_ref, o_abs, N),
                               tag + "out")

    # ---- backward, from the kernel's probs and rnorm; then on |.|
    def chain(x_, g_, sign):
        dP = torch.matmul(g_, x_.transpose(-1, -2))
        t = (P * dP).sum(-1, keepdim=True)
        dS = (alpha * P * (dP + sign * t)).masked_fill(const, 0.0)
        dSr = dS * r[:, :, None, :]
        dv = torch.matmul(P.transpose(-1, -2), g_)
        dq = torch.matmul(dSr, x_)
        dkh = torch.matmul(dS.transpose(-1, -2), x_)
        c = r * r * (dkh * x_).sum(-1)
        c = torch.where(r >= 0.999e12, torch.zeros_like(c), c)
        dk = r[..., None] * (dkh + sign * x_ * c[..., None])
        return (dk + dv + dq).permute(0, 2, 1, 3)

    d_ref = chain(x, g, -1.0)
    d_abs = chain(ax, ag, 1.0)
    fig["dLevels"] = assert_within(dLev, d_ref, 5 * U * d_abs,
                                   tag + "dLevels")
    # the zero row's gradient is dkhat / eps: huge, finite, and checked
    assert float(d_ref[0, 1, 0].abs().max()) > 1e6
    print("consensus " + tag + " ".join(
        "%s %.3f" % kv for kv in fig.items()))


# fused softmax (N == 256): d = 192, 320 leave a partial 256-column chunk
# in the fused AV; unfused: N % 8 == 0 vector softmax, N = 9 scalar softmax
SHAPES = [(256, 64), (256, 192), (256, 320), (16, 64), (72, 64), (9, 8)]


@pytest.mark.parametrize("attend_self", [False, True])
@pytest.mark.parametrize("N,d", SHAPES)
def test_consensus_stages(N, d, attend_self):
    check_consensus(N, d, attend_self, None)


@pytest.mark.parametrize("attend_self", [False, True])
def test_consensus_stages_radius_mask(attend_self):
    check_consensus(256, 64, attend_self, _radius_mask(16, 3))


def test_consensus_stages_unfused_av():
    """N = 256 with the AV product as its own NN GEMM (GLOM_NO_FUSE_AV is
    read per call, but set for a whole child process so nothing else in
    this one sees it)."""
    env = dict(os.environ, GLOM_NO_FUSE_AV="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "consensus N256 d64" in r.stdout
    print(r.stdout.strip())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    assert os.environ.get("GLOM_NO_FUSE_AV")
    check_consensus(256, 64, False, None)
    check_consensus(256, 64, False, _radius_mask(16, 3))
