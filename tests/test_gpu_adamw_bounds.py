"""Fused AdamW (k_grad_norm_part / fin, k_adamw, k_adamw_sched) per element
against fp64.

One step from a given state is compared with ``adamw_step_ref`` of
tests/_stream_util.py, whose docstring derives the tolerance of exp_avg,
exp_avg_sq and the master from the roundings of the step; the clip norm is
compared with the fp64 norm, and the clip scale of the step reference is
then computed from the kernel's own norm (stage by stage, as in
test_gpu_bounds_consensus.py). Chained steps are checked each against the
reference from the kernel's own previous state, and once at the end against
torch.optim.AdamW on fp64 clones with the tolerance carried along.

Tensors: (3,); (64, 9, 5); 2 * 524288 + 777 elements, so that the grid-stride
loops of the update (524288 per pass) and of the norm (262144 per pass) both
make a last, partial pass; gradients of 1e-8, where eps decides the update;
and gradients with planted exact zeros.
"""

import pytest
import torch

from _bounds_util import assert_within
from _stream_util import (BF, STEP_STRIDE, U32, adamw_step_ref,
                          check_fused_step, clip_scale, f32, norm_ref,
                          opt_snapshot)

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
SHAPES = [(3,), (64, 9, 5), (2 * STEP_STRIDE + 777,), (2880,), (1000,)]
GSCALE = [3.0, 3.0, 3.0, 1e-8, 3.0]
WDS = [1e-2, 0.0, 1e-2, 5e-2, 1e-2]
SCALES = [0.5, 1.0, 1.0, 1.0, 1.0]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _problem(t, seed=0):
    """Masters, bf16 params, gradients and a state as t - 1 steps leave it.
    The 1e-8 gradients keep |g| >= 5e-9 so that nothing the step computes
    from them is subnormal; the last tensor has every third gradient +0 or
    -0."""
    g = _gen(seed + t % 97)
    rn = lambda s: torch.randn(s, device=DEV, generator=g)
    masters, grads, m1s, m2s = [], [], [], []
    for i, (s, gs) in enumerate(zip(SHAPES, GSCALE)):
        masters.append(rn(s))
        gr = rn(s)
        if gs < 1:
            gr = torch.sign(gr) * (gr.abs() + 0.5)
        gr = (gr * gs).to(BF)
        if i == 4:
            gr[::3] = 0.0
            gr[::6] = -0.0
        grads.append(gr)
        m1s.append(rn(s) * gs * (0.0 if t == 1 else 0.3))
        m2 = (rn(s) * gs).pow(2) * (1 - B2 ** (t - 1))
        if i == 4:
            m2[::6] = 0.0          # v == 0 exactly: the update is 0 / eps
        m2s.append(m2)
    params = [m.to(BF) for m in masters]
    return params, masters, grads, m1s, m2s


def _make(kind, params, masters, clip):
    from glom_pytorch_amd.ops.optim import FusedAdamW
    n = len(params)
    if kind == "sched":
        opt = FusedAdamW(params, masters, lr=LR, betas=(B1, B2), eps=EPS,
                         weight_decay=WDS[:n], lr_scale=SCALES[:n],
                         max_grad_norm=clip)
        assert opt._uses_device_lr()
        return opt, [f32(LR) * s for s in SCALES[:n]], WDS[:n]
    opt = FusedAdamW(params, masters, lr=LR, betas=(B1, B2), eps=EPS,
                     weight_decay=1e-2, max_grad_norm=clip)
    assert not opt._uses_device_lr()
    return opt, [LR] * n, [1e-2] * n


def _set_state(opt, m1s, m2s, t):
    for a, b, m1, m2 in zip(opt.exp_avg, opt.exp_avg_sq, m1s, m2s):
        a.copy_(m1)
        b.copy_(m2)
    opt._step_dev.fill_(float(t - 1))


@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000])
@pytest.mark.parametrize("kind", ["arg", "sched"])
def test_one_step_from_a_given_state(kind, t, clip):
    params, masters, grads, m1s, m2s = _problem(t)
    opt, lrs, wds = _make(kind, params, masters, clip)
    _set_state(opt, m1s, m2s, t)
    before = opt_snapshot(opt)
    for p, g in zip(params, grads):
        p.grad = g
    opt.step()
    worst = check_fused_step(opt, before, grads, t, lrs, wds, kind)
    print("adamw %s t=%d clip=%g err/tol norm %.3f exp_avg %.3f "
          "exp_avg_sq %.3f master %.3f" % ((kind, t, clip) + tuple(worst)))
    assert opt.steps_done() == t
    # every master moved, the last grid-stride pass included
    for b, m in zip(before, masters):
        assert not torch.equal(b[2].view(-1)[-8:], m.view(-1)[-8:])


@pytest.mark.parametrize("kind", ["arg", "sched"])
def test_parameter_without_gradient_is_left_alone(kind):
    params, masters, grads, m1s, m2s = _problem(10, seed=1)
    keep = [0, 1, 3]                     # without the 1 M-element tensor
    params, masters, grads, m1s, m2s = (
        [x[i] for i in keep] for x in (params, masters, grads, m1s, m2s))
    opt, lrs, wds = _make(kind, params, masters, 1.0)
    _set_state(opt, m1s, m2s, 10)
    before = opt_snapshot(opt)
    p_before = [p.clone() for p in params]
    grads[1] = None
    for p, g in zip(params, grads):
        p.grad = g
    opt.step()
    # the norm inside is taken over the present gradients only
    check_fused_step(opt, before, grads, 10, lrs, wds, kind)
    for got, want in zip((opt.exp_avg[1], opt.exp_avg_sq[1], masters[1]),
                         before[1]):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(params[1].view(torch.int16),
                       p_before[1].view(torch.int16))
    assert opt.steps_done() == 10


@pytest.mark.parametrize("kind", ["arg", "sched"])
def test_five_chained_steps(kind):
    """Each step against the reference from the kernel's own previous
    state; at the end against torch.optim.AdamW on fp64 clones (fp32-rounded
    hyperparameters as Python floats, clip_grad_norm_ on the fp64 grads).
    The end tolerance is the one-step tolerances summed along torch's
    trajectory: each step's bound takes the bound on its incoming state
    (d_in), so errors in exp_avg / exp_avg_sq carry with b1 / b2 and the
    norm's own tolerance enters the clip scale."""
    steps, clip = 5, 1.0
    g = _gen(5)
    shapes = [(512, 17), (3,), (64, 9, 5)]
    masters = [torch.randn(s, device=DEV, generator=g) for s in shapes]
    params = [m.to(BF) for m in masters]
    opt, lrs, wds = _make(kind, params, masters, clip)
    ref_p = [m.double().clone().requires_grad_(True) for m in masters]
    groups = [{"params": [q], "lr": lr, "weight_decay": f32(wd)}
              for q, lr, wd in zip(ref_p, lrs, wds)]
    topt = torch.optim.AdamW(groups, lr=f32(LR), betas=(f32(B1), f32(B2)),
                             eps=f32(EPS))
    for grp, lr in zip(topt.param_groups, lrs):
        grp["lr"] = f32(lr)
    chain = [(torch.zeros_like(q), torch.zeros_like(q), q.detach().clone())
             for q in ref_p]
    d_in = [None] * len(shapes)
    for t in range(1, steps + 1):
        grads = [(torch.randn(s, device=DEV, generator=g) * 3).to(BF)
                 for s in shapes]
        before = opt_snapshot(opt)
        for p, gr in zip(params, grads):
            p.grad = gr
        opt.step()
        check_fused_step(opt, before, grads, t, lrs, wds, kind)
        norm64, norm_tol = norm_ref(grads)
        for i, gr in enumerate(grads):
            chain[i], d_in[i] = adamw_step_ref(
                gr, *chain[i], lrs[i], B1, B2, EPS, wds[i], t,
                scale=clip_scale(norm64, clip),
                e_scale=3 * U32 + norm_tol / norm64, d_in=d_in[i])
            ref_p[i].grad = gr.double()
        torch.nn.utils.clip_grad_norm_(ref_p, f32(clip))
        topt.step()
    worst = [0.0, 0.0, 0.0]
    for i, q in enumerate(ref_p):
        st = topt.state[q]
        want = (st["exp_avg"], st["exp_avg_sq"], q.detach())
        got = (opt.exp_avg[i], opt.exp_avg_sq[i], masters[i])
        for k in range(3):
            # the reference chain is torch's step, to fp64 roundoff (of
            # the terms, hence against the tensor's largest magnitude)
            assert ((chain[i][k] - want[k]).abs()
                    <= 1e-13 * want[k].abs().max()).all(), (i, k)
            worst[k] = max(worst[k], assert_within(
                got[k], want[k], d_in[i][k], "torch fp64 %d/%d" % (i, k)))
    print("adamw %s 5 steps vs torch fp64 err/tol %.3f %.3f %.3f"
          % ((kind,) + tuple(worst)))
    assert opt.steps_done() == steps


@pytest.mark.parametrize("kind", ["arg", "sched"])
def test_more_than_24_tensors_is_an_error(kind):
    from glom_pytorch_amd.ops.optim import FusedAdamW
    g = _gen(6)
    masters = [torch.randn(16, device=DEV, generator=g) for _ in range(25)]
    params = [m.to(BF) for m in masters]
    kw = dict(lr_scale=[0.5] + [1.0] * 24) if kind == "sched" else {}
    opt = FusedAdamW(params, masters, lr=LR, max_grad_norm=1.0, **kw)
    start = [m.clone() for m in masters]
    for p in params:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="24"):
        opt.step()
    torch.cuda.synchronize()
    assert opt.steps_done() == 0
    for m, s, a, b in zip(masters, start, opt.exp_avg, opt.exp_avg_sq):
        assert torch.equal(m, s)
        assert not a.any() and not b.any()
