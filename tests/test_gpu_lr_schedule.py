"""Device-resident learning-rate schedule and per-tensor groups of the fused
AdamW (``k_grad_norm_fin_sched`` / ``k_adamw_sched``), and the trainer on
top: an lr assignment that takes effect on a graphed trainer, the schedule,
resume."""

import pytest
import torch

from conftest import SMALL, SMALL_BATCH, SMALL_ITERS
from glom_pytorch_amd import Glom
from glom_pytorch_amd.ops.optim import LRSchedule

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"
# the tensor shapes of test_fused_adamw_matches_torch: not a multiple of a
# wave, of 8, or of the grid stride
SHAPES = [(512, 17), (3,), (128,), (64, 9, 5)]


def _rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _tensors(seed=0, steps=5):
    torch.manual_seed(seed)
    base = [torch.randn(s, device=DEV) for s in SHAPES]
    params = [b.to(torch.bfloat16) for b in base]
    masters = [p.float() for p in params]
    grads_seq = [[(torch.randn(s, device=DEV) * 3).to(torch.bfloat16)
                  for s in SHAPES] for _ in range(steps)]
    return params, masters, grads_seq


def _run(opt, params, grads_seq):
    for grads in grads_seq:
        for p, g in zip(params, grads):
            p.grad = g
        opt.step()


# ------------------------------ optimizer ------------------------------ #

@pytest.mark.parametrize("clip", [1.0, 0.0])
def test_sched_kernels_bit_identical_to_kernel_arg_path(clip):
    """Constant schedule, scalar wd, lr_scale 1: the device-lr kernels are
    the kernel-argument kernels' arithmetic, bit for bit."""
    from glom_pytorch_amd.ops.optim import FusedAdamW
    pa, ma, grads_seq = _tensors()
    pb, mb = [p.clone() for p in pa], [m.clone() for m in ma]
    start = [m.clone() for m in ma]
    old = FusedAdamW(pa, ma, lr=1e-2, max_grad_norm=clip)
    new = FusedAdamW(pb, mb, lr=1e-2, max_grad_norm=clip,
                     schedule=LRSchedule("constant", warmup_steps=0))
    assert not old._uses_device_lr() and new._uses_device_lr()
    _run(old, pa, grads_seq)
    _run(new, pb, grads_seq)
    for i in range(len(SHAPES)):
        assert torch.equal(ma[i], mb[i]), i
        assert torch.equal(old.exp_avg[i], new.exp_avg[i]), i
        assert torch.equal(old.exp_avg_sq[i], new.exp_avg_sq[i]), i
        assert torch.equal(pa[i], pb[i]), i
        assert not torch.equal(ma[i], start[i]), i
    assert old.steps_done() == new.steps_done() == len(grads_seq)
    assert new.current_lr() == pytest.approx(1e-2, rel=1e-7)


@pytest.mark.parametrize("clip", [1.0, 0.0])
def test_sched_groups_match_torch(clip):
    """Cosine schedule, wd 0 on the 1-D tensors, lr_scale 0.5 on one
    tensor, against torch.optim.AdamW with matching groups whose lr is set
    per step from LRSchedule.factor."""
    from glom_pytorch_amd.ops.optim import FusedAdamW
    steps, lr = 8, 1e-2
    params, masters, grads_seq = _tensors(steps=steps)
    ref = [m.clone() for m in masters]
    sc = LRSchedule("cosine", warmup_steps=3, total_steps=6, min_ratio=0.1)
    wd = [0.0 if len(s) == 1 else 1e-2 for s in SHAPES]
    scale = [0.5, 1.0, 1.0, 1.0]

    fused = FusedAdamW(params, masters, lr=lr, weight_decay=wd,
                       lr_scale=scale, max_grad_norm=clip, schedule=sc)
    # each step also per element against fp64, from the state before it and
    # the learning rate the device evaluated for it
    from _stream_util import check_fused_step, opt_snapshot
    for t, grads in enumerate(grads_seq, 1):
        before = opt_snapshot(fused)
        _run(fused, params, [grads])
        lr_t = fused.current_lr()
        check_fused_step(fused, before, grads, t, [lr_t * s for s in scale],
                         wd)

    groups = [{"params": [ref[0]], "weight_decay": 1e-2, "scale": 0.5},
              {"params": [ref[1], ref[2]], "weight_decay": 0.0, "scale": 1.0},
              {"params": [ref[3]], "weight_decay": 1e-2, "scale": 1.0}]
    topt = torch.optim.AdamW(groups, lr=lr, foreach=True)
    for k, grads in enumerate(grads_seq):
        for m, g in zip(ref, grads):
            m.grad = g.float()
        if clip:
            torch.nn.utils.clip_grad_norm_(ref, clip)
        for g in topt.param_groups:
            g["lr"] = lr * g["scale"] * sc.factor(k)
        topt.step()
        topt.zero_grad(set_to_none=True)

    for m, r in zip(masters, ref):
        assert _rel_err(m, r) < 1e-4, (m.shape, _rel_err(m, r))
    for p, r in zip(params, ref):
        assert _rel_err(p, r.to(torch.bfloat16)) < 1e-2
    assert fused.steps_done() == steps


@pytest.mark.parametrize("kind,W,T,m", [
    ("constant", 3, 8, 0.1),
    ("linear", 3, 8, 0.1),
    ("cosine", 3, 8, 0.1),
    ("cosine", 0, 7, 0.0),      # no warmup, decays to exactly zero
])
def test_device_schedule_matches_specification(kind, W, T, m):
    """lr_t on the device against the float64 specification. The bound is
    derived: under ten fp32 roundings (6e-8 each) of O(1) quantities plus
    cosf's few ulp stays below 1e-6; absolute (in units of the base lr)
    because 1 + cos cancels near the end of the curve."""
    from glom_pytorch_amd.ops.optim import FusedAdamW
    lr = 3e-3
    sc = LRSchedule(kind, warmup_steps=W, total_steps=T, min_ratio=m)
    torch.manual_seed(0)
    params = [torch.randn(33, device=DEV).to(torch.bfloat16)]
    opt = FusedAdamW(params, [params[0].float()], lr=lr, schedule=sc)
    for s in range(T + 3):
        params[0].grad = torch.randn_like(params[0])
        opt.step()
        got, want = opt.current_lr(), lr * sc.factor(s)
        assert abs(got - want) <= 1e-6 * lr, (kind, s, got, want)
    assert opt.steps_done() == T + 3


def test_state_dict_two_groups_interchange():
    from glom_pytorch_amd.ops.optim import FusedAdamW
    torch.manual_seed(1)
    shapes = [(16, 8), (8,), (4, 8), (5,)]
    params = [torch.randn(s, device=DEV).to(torch.bfloat16) for s in shapes]
    masters = [p.float() for p in params]
    wd = [1e-2, 0.0, 1e-2, 0.0]
    fused = FusedAdamW(params, masters, lr=3e-3, weight_decay=wd,
                       max_grad_norm=1.0)
    for _ in range(3):
        for p in params:
            p.grad = torch.randn_like(p)
        fused.step()
    sd = fused.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1], [2, 3]]
    assert [g["weight_decay"] for g in sd["param_groups"]] == [1e-2, 0.0]
    assert all(g["lr"] == 3e-3 for g in sd["param_groups"])

    clones = [m.clone().requires_grad_(True) for m in masters]
    topt = torch.optim.AdamW(
        [{"params": [clones[0], clones[2]], "weight_decay": 1e-2},
         {"params": [clones[1], clones[3]], "weight_decay": 0.0}], lr=3e-3)
    topt.load_state_dict(sd)
    # torch now holds tensor 2's moments as its second parameter
    assert torch.allclose(topt.state[clones[2]]["exp_avg"],
                          fused.exp_avg[2])
    fused2 = FusedAdamW(params, [m.clone() for m in masters], lr=1e-3,
                        weight_decay=wd)
    fused2.load_state_dict(topt.state_dict())
    for a, b in zip(fused.exp_avg, fused2.exp_avg):
        assert torch.allclose(a, b)
    for a, b in zip(fused.exp_avg_sq, fused2.exp_avg_sq):
        assert torch.allclose(a, b)
    assert fused2.steps_done() == 3
    assert fused2.lr == 3e-3
    # a single-group optimizer refuses the two-group state
    with pytest.raises(ValueError):
        FusedAdamW(params, [m.clone() for m in masters]).load_state_dict(sd)


# ------------------------------- trainer ------------------------------- #

def _trainer(graph, seed=0, noise_std=0.0, **kw):
    from glom_pytorch_amd.parallel.trainer import DenoisingTrainer
    torch.manual_seed(seed)
    m = Glom(**SMALL).to(DEV, torch.bfloat16)
    return DenoisingTrainer(m, lr=1e-3, noise_std=noise_std,
                            graph_step=graph, **kw)


def _same_init(dst, src):
    dst.model.load_state_dict(src.model.state_dict())
    dst.decoder.load_state_dict(src.decoder.state_dict())
    with torch.no_grad():
        for mw, q in zip(dst.master, dst._params):
            mw.copy_(q.float())


def _img():
    return torch.randn(SMALL_BATCH, 3, 32, 32, device=DEV).to(torch.bfloat16)


def _graph_entry(tr):
    assert len(tr._graphs) == 1
    entry = next(iter(tr._graphs.values()))
    assert entry is not False, "capture fell back to eager"
    return entry


def test_lr_assignment_takes_effect_on_graphed_trainer():
    """The trap: a captured step bakes lr in as a kernel argument. Assigning
    opt.lr on a trainer that has been replaying its graph must take effect
    on the very next step. (It does so by launching that step eagerly with
    lr read from device memory; the captured entry is left alone.)"""
    img = _img()
    tr = _trainer(graph=True)
    for _ in range(2):
        tr.step(img, iters=SMALL_ITERS)
    entry = _graph_entry(tr)

    tr.opt.lr = 0.0
    masters = [m.clone() for m in tr.master]
    params = [q.detach().clone() for q in tr._params]
    exp_avg = [t.clone() for t in tr.opt.exp_avg]
    tr.step(img, iters=SMALL_ITERS)
    for i, (a, b) in enumerate(zip(tr.master, masters)):
        assert torch.equal(a, b), i
    for i, (a, b) in enumerate(zip(tr._params, params)):
        assert torch.equal(a, b), i
    assert any(not torch.equal(a, b)
               for a, b in zip(tr.opt.exp_avg, exp_avg))
    assert _graph_entry(tr) is entry
    assert tr.current_lr() == 0.0

    tr.opt.lr = 1e-3
    tr.step(img, iters=SMALL_ITERS)
    assert any(not torch.equal(a, b) for a, b in zip(tr.master, masters))
    assert _graph_entry(tr) is entry
    assert tr.opt.steps_done() == 4


def test_trainer_follows_device_schedule():
    """A scheduled trainer launches its steps eagerly whatever graph_step
    says (nothing is captured), follows the specification within the bound
    of test_device_schedule_matches_specification, and is reproducible."""
    sc = LRSchedule("cosine", warmup_steps=4, total_steps=8, min_ratio=0.1)
    img = _img()
    ta = _trainer(graph=False, lr_schedule=sc)
    tb = _trainer(graph=True, lr_schedule=sc)
    _same_init(tb, ta)
    losses_a = [ta.step(img, iters=SMALL_ITERS) for _ in range(10)]
    losses_b = []
    for s in range(10):
        losses_b.append(tb.step(img, iters=SMALL_ITERS))
        got, want = tb.current_lr(), 1e-3 * sc.factor(s)
        assert abs(got - want) <= 1e-6 * 1e-3, (s, got, want)
    assert tb._graphs == {}
    assert ta.opt.steps_done() == tb.opt.steps_done() == 10
    assert losses_a == losses_b
    for a, b in zip(ta.master, tb.master):
        assert torch.equal(a, b)


def test_resume_continues_schedule(tmp_path):
    sc = LRSchedule("cosine", warmup_steps=2, total_steps=8, min_ratio=0.1)
    img = _img()
    path = str(tmp_path / "ck.pt")
    ta = _trainer(graph=False, noise_std=0.5, lr_schedule=sc, no_decay=True)
    for _ in range(5):
        ta.step(img, iters=SMALL_ITERS)
    ta.save_checkpoint(path)
    lrs_a = []
    for _ in range(3):
        ta.step(img, iters=SMALL_ITERS)
        lrs_a.append(ta.current_lr())

    tb = _trainer(graph=False, noise_std=0.5, no_decay=True)
    _same_init(tb, ta)
    tb.load_checkpoint(path)
    assert tb.lr_schedule == sc
    lrs_b = []
    for _ in range(3):
        tb.step(img, iters=SMALL_ITERS)
        lrs_b.append(tb.current_lr())
    assert lrs_b == lrs_a
    for s, got in zip((5, 6, 7), lrs_b):
        assert abs(got - 1e-3 * sc.factor(s)) <= 1e-6 * 1e-3
    assert tb.opt.steps_done() == 8
    for i, (a, b) in enumerate(zip(ta.master, tb.master)):
        assert torch.equal(a, b), i
    for (n, pa), (_, pb) in zip(ta.model.named_parameters(),
                                tb.model.named_parameters()):
        assert torch.equal(pa, pb), n

    with pytest.raises(ValueError):
        _trainer(graph=False, no_decay=False).load_checkpoint(path)
