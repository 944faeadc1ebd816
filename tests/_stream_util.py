"""fp64 references and per-element bounds for the streaming kernels between
the GEMMs (level mix, backward level chain, fixed-order reductions) and for
the fused AdamW. No GPU dependency: everything works on the device of its
arguments. Written from the specification (the eager model's
``(prev + bu + pad(td) + cons) / c``, torch.optim.AdamW, the docstrings in
``aux_kernels.h`` / ``native_ops.h``), not from the kernels.

``U`` = 2^-8 is the bf16 unit roundoff, ``U32`` = 2^-24 the f32 one.

Exactness on integer probes. With operands from ``int_probe(.., -256, 256)``
every f32 partial sum of four of them is an integer below 2^24, hence exact;
n / 4 is exact; and bf16(f32(n / 3)) equals n / 3 rounded once to bf16 for
every integer |n| <= 1024, as does bf16(f32(v / c)) for every finite bf16 v
and c in {3, 4} (both checked exhaustively in test_stream_bounds_cpu.py: the
f32 quotient never lands on a bf16 tie it was not already on). So mix
forward and backward, add4 and grad_merge are compared with ``assert_exact``.
Column sums and dpos of probes in [-8, 8] stay below 2^24 up to 2^21 rows.
"""

import numpy as np
import torch
import torch.nn.functional as F

from _bounds_util import U, assert_within, gemm_tol, round_once

U32 = 2.0 ** -24
BF = torch.bfloat16
NAN_BITS = 0x7FC1        # a quiet NaN with a payload bit
NEG_ZERO = -32768        # 0x8000 as int16


def f32(x):
    """A Python float rounded to fp32: what a kernel's float argument holds."""
    return float(np.float32(x))


def nan_like(x):
    return torch.full_like(x.view(torch.int16), NAN_BITS).view(BF)


def level_c(L, device):
    c = torch.full((1, 1, L, 1), 4.0, dtype=torch.float64, device=device)
    c[:, :, L - 1] = 3.0
    return c


# ------------------------------ level mix ------------------------------ #

def mix_ref(prev, bu, td, cons, bu0=None):
    """(prev + bu + pad(td) + cons) / c_l with c = [4, .., 4, 3]; td has
    L - 1 level slots and nothing is added at the top one. bu0 (B,N,d), if
    given, is level 0 of the bottom-up term and slice 0 of ``bu`` is not
    read. Returns (ref64, tol64).

    Bound for real operands: the kernel adds the (up to) four operands in
    f32, divides by c_l in f32 and rounds to bf16 once. Each of the at most
    three adds errs by at most 2^-24 of a partial sum, itself at most
    S = sum |operand|, and the divide by 2^-24 of the result, at most
    S / c_l: together 4 * 2^-24 * S / c_l to first order. The bf16 rounding
    adds U * |value|:
        tol = U * |ref| + 4 * 2^-24 * S / c_l
    """
    L = prev.shape[2]
    b = bu.double()
    if bu0 is not None:
        b = torch.cat([bu0.double().unsqueeze(2), b[:, :, 1:]], dim=2)
    tdp = F.pad(td.double(), (0, 0, 0, 1), value=0.0)
    c = level_c(L, prev.device)
    ref = (prev.double() + b + tdp + cons.double()) / c
    S = prev.double().abs() + b.abs() + tdp.abs() + cons.double().abs()
    return ref, U * ref.abs() + 4 * U32 * S / c


def mix_next_ref(out, pos):
    """What the fused mix emits for the next iteration, from the stored
    bf16 ``out`` (B,N,L,d) and pos (N,d):
      td_next[b,n,l-1] = out[b,n,l] + pos[n]  (l >= 1; one f32 add of two
        bf16 values and one bf16 rounding: exact on integer probes)
      rn_next[b,l,n] = 1 / max(||out[b,n,l]||_2, 1e-12)
    Returns (td_next64, rn64, rn_tol64). rn bound: the d squares of bf16
    values are exact in f32; d - 1 adds in any order, the square root, the
    divide and the clamp constant's own rounding make at most d + 2
    roundings of 2^-24 (the square root halves what precedes it; no credit
    is taken for that): (d + 4) * 2^-24 relative.
    """
    d = out.shape[3]
    o = out.double()
    td_next = o[:, :, 1:] + pos.double().view(1, pos.shape[0], 1, d)
    nrm = o.pow(2).sum(-1).sqrt().clamp_min(f32(1e-12))
    rn = (1.0 / nrm).permute(0, 2, 1).contiguous()
    return td_next, rn, (d + 4) * U32 * rn


def mix_bwd_ref(dout):
    """dmix = dout / c_l; dtd = dmix[:, :, :L-1]. One f32 divide of a bf16
    value and one bf16 rounding, which equals the fp64 quotient rounded once
    (module docstring), so both compare with ``assert_exact`` for any
    finite input."""
    L = dout.shape[2]
    dmix = dout.double() / level_c(L, dout.device)
    return dmix, dmix[:, :, :L - 1]


def merge_ranges(lo, L):
    """Level ranges of (dmix, bottom-up, top-down, dAttn) of a step whose
    first live level is lo, and the first level that is not dead."""
    return ((lo, L), (max(lo, 1) - 1, L - 1), (lo + 1, L), (lo, L)), \
        max(lo - 1, 0)


def plant_zeros(xs, gen):
    """The zero patterns of test_gpu_bwd_merge._merge_inputs, planted in
    place into four same-shaped tensors: +0 in one operand, -0 in one, all
    four -0 (the only way to a -0 sum), all four +0, and -0, -0, +0, -0
    (which must give +0)."""
    flat = [x.view(-1) for x in xs]
    n = flat[0].numel()
    pick = torch.randperm(n, device=gen.device, generator=gen)
    k = max(n // 16, 1)
    for i, f in enumerate(flat):
        f[pick[i * k:(i + 1) * k]] = 0.0
        f[pick[(4 + i) * k:(5 + i) * k]] = -0.0
    for i, f in enumerate(flat):
        f[pick[8 * k:9 * k]] = -0.0
        f[pick[9 * k:10 * k]] = 0.0
        f[pick[10 * k:11 * k]] = 0.0 if i == 2 else -0.0
    return xs


def poison_outside(xs, lo, L):
    """Copies of the four contributions with NaNs outside their ranges."""
    out = []
    for x, (r0, r1) in zip(xs, merge_ranges(lo, L)[0]):
        y = nan_like(x)
        y[:, :, r0:r1] = x[:, :, r0:r1]
        out.append(y)
    return out


def merge_ref(xs, lo, posz):
    """Backward merge of the four contributions (B,N,L,d): each is taken
    inside its level range and is +0 outside it (so what lies there, NaNs
    included, is never read); the four are added in the order given; levels
    below max(lo - 1, 0) are +0. posz adds +0 to the sum, which turns an
    exact -0 into +0 and changes nothing else.
        out       = round_once(sum)
        dmix_next = round_once(round_once(sum) / c_l)     (two roundings)
    Returns (sum64, next64, S64, first): next64 is computed from the
    once-rounded sum, S = sum of |summand| for the real-operand bound
        tol_out = U * |sum| + 3 * 2^-24 * S          (three f32 adds)
    and ``first`` the first level at which dmix_next is specified.
    """
    L = xs[0].shape[2]
    ranges, first = merge_ranges(lo, L)
    lev = torch.arange(L, device=xs[0].device).view(1, 1, L, 1)
    total, S = None, None
    for x, (r0, r1) in zip(xs, ranges):
        live = ((lev >= r0) & (lev < r1)).expand_as(x)
        v = torch.where(live, x.double(),
                        torch.zeros_like(x, dtype=torch.float64))
        total = v if total is None else total + v
        S = v.abs() if S is None else S + v.abs()
    dead = (lev < first).expand_as(total)
    total = torch.where(dead, torch.zeros_like(total), total)
    if posz:
        total = total + 0.0
    nxt = round_once(total, BF).double() / level_c(L, total.device)
    return total, nxt, S, first


def merge_tol(total, S):
    return U * total.abs() + 3 * U32 * S


# --------------------------- fixed-order sums --------------------------- #

def colsum_ref(x):
    """(M, C) -> (C,) and the tolerance for real operands: M - 1 f32 adds
    in a fixed order plus one bf16 rounding, ``gemm_tol`` with K = M.
    Integer probes in [-8, 8] give exact f32 sums for M < 2^21."""
    x = x.double()
    ref = x.sum(0)
    return ref, gemm_tol(ref, x.abs().sum(0), x.shape[0])


def db2_ref(dmix, lo):
    """dB2 of both FF nets from dmix (B,N,L,d) with first live level lo:
    the sum over the B*N rows of the columns [lo*d, L*d), +0 for the dead
    columns, whose input is never read. Returns (bu64 (L*d,), td64
    ((L-1)*d,), tol_bu64): the top-down vector is the bottom-up one without
    the top level."""
    B, N, L, d = dmix.shape
    lev = torch.arange(L, device=dmix.device).view(1, 1, L, 1)
    x = torch.where((lev >= lo).expand_as(dmix), dmix.double(),
                    torch.zeros_like(dmix, dtype=torch.float64))
    bu, tol = colsum_ref(x.reshape(B * N, L * d))
    return bu, bu[:(L - 1) * d], tol


def dpos_ref(dlev, l0):
    """dPos[n, q] = sum over b and levels l0..L-1 of dLevels[b, n, l, q];
    l0 >= L: all +0. Levels below l0 are not read. Tolerance as colsum with
    K = B * (L - l0) summands."""
    B, N, L, d = dlev.shape
    x = dlev.double()[:, :, l0:]
    ref = x.sum((0, 2))
    return ref, gemm_tol(ref, x.abs().sum((0, 2)), B * max(L - l0, 0))


# -------------------------------- AdamW -------------------------------- #

NORM_STRIDE = 1024 * 256     # elements one pass of the norm grid covers
STEP_STRIDE = 2048 * 256     # elements one pass of the update grid covers


def norm_ref(grads):
    """fp64 L2 norm over all gradients and its tolerance. All summands are
    non-negative, so a sum of them computed with `depth` roundings on the
    longest path errs by at most depth * 2^-24 relative, whatever the
    order; the square root halves that and rounds once more:
        tol = (depth / 2 + 1) * 2^-24 * norm
    depth = sum over tensors of ceil(n / 262144) (one thread's fma chain
    across all tensors) + 24 (per stage a 6-step wave reduce and a 4-term
    cross-wave sum, in both stages, and 4 partials per thread in the
    finish)."""
    s = sum(g.double().pow(2).sum() for g in grads)
    depth = sum(-(-g.numel() // NORM_STRIDE) for g in grads) + 24
    norm = float(s.sqrt())
    return norm, (depth / 2 + 1) * U32 * norm


def clip_scale(norm, max_norm):
    """torch's clip_grad_norm_ coefficient, min(1, max_norm / (norm +
    1e-6)), with the constants as the kernel holds them (fp32)."""
    if not max_norm > 0:
        return 1.0
    return min(1.0, f32(max_norm) / (norm + f32(1e-6)))


def adamw_step_ref(g, m1, m2, p, lr, b1, b2, eps, wd, t, scale=1.0,
                   e_scale=0.0, d_in=None):
    """One torch.optim.AdamW step in fp64 from the state (m1, m2, p), on the
    gradient g * scale, at step count t (the count after this step):
        m = b1 m1 + (1 - b1) g          v = b2 m2 + (1 - b2) g^2
        p' = p (1 - lr wd) - (lr / (1 - b1^t)) m / (sqrt(v / (1 - b2^t)) + eps)
    The hyperparameters are rounded to fp32 first, as kernel arguments are.
    Returns ((m, v, p'), (tol_m, tol_v, tol_p)).

    Bound, u = 2^-24, first order, then times (1 + 2^-10) for the products
    of these terms. e_scale is the relative error of the clip scale the
    kernel used against `scale` (3 u with clipping on: the add of 1e-6, the
    divide, and the product g * scale; 0 with clipping off, where the
    product is exact). d_in = (d_m1, d_m2, d_p) are tolerances on the
    incoming state, for chaining; they enter with the factors b1, b2 and
    (1 - lr wd).
      m:  one fma rounding, and (1 - b1) * g carries e_scale plus the
          roundings of 1 - b1 and of the product:
            tol_m = u |m| + (e_scale + 2u) |(1 - b1) g| + b1 d_m1
      v:  as m with two products by g:
            tol_v = u |v| + (2 e_scale + 3u) (1 - b2) g^2 + b2 d_m2
      bias corrections: pow is within 1 ulp (2u relative) of b^t and the
          subtraction rounds once: e_bc = u (1 + 2 b^t / (1 - b^t))
      step size lr / bc1: e_ss = e_bc1 + u
      vhat = v * (1 / bc2): e_vhat = tol_v / v + e_bc2 + 2u
      s = sqrt(vhat): d_s = s (e_vhat / 2 + u)
      den = s + eps:  d_den = d_s + u den
      num = step_size * m: d_num = step_size tol_m + |num| (e_ss + u)
      upd = num / den: d_upd = d_num / den + |upd| (d_den / den + u)
      p1 = p * decay, decay one fma: d_p1 = 2u |p1| + decay d_p
      p' = p1 - upd: tol_p = d_p1 + d_upd + u |p'|
    """
    u = U32
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, b1, b2, eps, wd))
    g64 = g.double() * scale
    z = torch.zeros_like(g64)
    d_m1, d_m2, d_p = d_in if d_in is not None else (z, z, z)
    m1, m2, p = m1.double(), m2.double(), p.double()

    gm = (1.0 - b1) * g64
    m = b1 * m1 + gm
    tol_m = u * m.abs() + (e_scale + 2 * u) * gm.abs() + b1 * d_m1
    gv = (1.0 - b2) * g64 * g64
    v = b2 * m2 + gv
    tol_v = u * v.abs() + (2 * e_scale + 3 * u) * gv + b2 * d_m2

    bt1, bt2 = b1 ** t, b2 ** t
    bc1, bc2 = 1.0 - bt1, 1.0 - bt2
    e_bc1 = u * (1 + 2 * bt1 / bc1)
    e_bc2 = u * (1 + 2 * bt2 / bc2)
    ss = lr / bc1
    e_ss = e_bc1 + u
    e_vhat = torch.where(v > 0, tol_v / v.clamp_min(1e-300), z) + e_bc2 + 2 * u
    s = (v / bc2).sqrt()
    d_s = s * (e_vhat / 2 + u)
    den = s + eps
    d_den = d_s + u * den
    num = ss * m
    d_num = ss * tol_m + num.abs() * (e_ss + u)
    upd = num / den
    d_upd = d_num / den + upd.abs() * (d_den / den + u)
    decay = 1.0 - lr * wd
    p1 = p * decay
    d_p1 = 2 * u * p1.abs() + abs(decay) * d_p
    pn = p1 - upd
    k = 1 + 2.0 ** -10
    tol_p = (d_p1 + d_upd) * k + u * pn.abs()
    return (m, v, pn), (tol_m * k, tol_v * k, tol_p)


def opt_snapshot(opt):
    """Clones of (exp_avg, exp_avg_sq, master) of every tensor."""
    return [(a.clone(), b.clone(), c.clone())
            for a, b, c in zip(opt.exp_avg, opt.exp_avg_sq, opt.masters)]


def check_fused_step(opt, before, grads, t, lrs, wds, what=""):
    """After one ``FusedAdamW.step()`` from the state `before` (an
    ``opt_snapshot``) on `grads` (None where a parameter had no gradient):
    the clip norm against fp64, then exp_avg, exp_avg_sq and the master of
    every present tensor against ``adamw_step_ref`` with the clip scale
    computed from the kernel's own norm, and param == bf16(master) bit for
    bit. lrs / wds: the per-tensor learning rate and weight decay of this
    step. Returns the worst err / tol of (norm, exp_avg, exp_avg_sq,
    master)."""
    present = [i for i, g in enumerate(grads) if g is not None]
    norm64, norm_tol = norm_ref([grads[i] for i in present])
    knorm = float(opt._norm.item())
    assert abs(knorm - norm64) <= norm_tol, (what, knorm, norm64, norm_tol)
    worst = [abs(knorm - norm64) / norm_tol if norm_tol else 0.0, 0.0, 0.0,
             0.0]
    clip = opt.max_grad_norm > 0
    scale = clip_scale(knorm, opt.max_grad_norm)
    for i in present:
        m1, m2, p = before[i]
        ref, tol = adamw_step_ref(
            grads[i], m1, m2, p, lrs[i], opt.betas[0], opt.betas[1], opt.eps,
            wds[i], t, scale=scale, e_scale=3 * U32 if clip else 0.0)
        got = (opt.exp_avg[i], opt.exp_avg_sq[i], opt.masters[i])
        for k, name in enumerate(("exp_avg", "exp_avg_sq", "master")):
            r = assert_within(got[k], ref[k], tol[k],
                              "%s %s[%d] t=%d" % (what, name, i, t))
            worst[k + 1] = max(worst[k + 1], r)
        assert torch.equal(opt.params[i].view(torch.int16),
                           opt.masters[i].to(BF).view(torch.int16)), (what, i)
    return worst
