"""Model-level cases shared by the token-hoist and mix-fusion tests: every
result of a forward, a training step or a trainer run must be
``torch.equal`` between a loop-invariant switch on and off, same build.

Each helper takes ``switch``, the ``glom_pytorch_amd.ops`` setter to flip
(``set_token_hoist`` / ``set_mix_fusion``), and the model configuration.
"""

import functools

import torch

from glom_pytorch_amd import Glom

DEV = "cuda:0"
BF = torch.bfloat16
ITERS = 6

# the issue's model; dim 256 keeps the standalone td_in / rnorm kernels
MODEL256 = dict(dim=256, levels=4, image_size=112, patch_size=7)
# the dim at which the level mix emits td_in / rnorm (N = 64: the unfused
# attention path, 16 mix blocks)
MODEL512 = dict(dim=512, levels=4, image_size=56, patch_size=7)

BWD_PATHS = {"fork3": {}, "fork4": {"GLOM_BWD_FORK": "4"},
             "single_stream": {"GLOM_NO_BWD_STREAMS": "1"}}
TRAIN_CASES = [(5, 3), (3, 3), (5, None)]
TRAIN_IDS = ["g5_lmin3", "g3_lmin3", "g5_nocone"]


def _key(cfg):
    return tuple(sorted(cfg.items()))


@functools.lru_cache(maxsize=None)
def _model_and_img(key):
    cfg = dict(key)
    torch.manual_seed(0)
    m = Glom(**cfg).to(DEV, BF)
    s = cfg["image_size"]
    img = torch.randn(2, 3, s, s, device=DEV).to(BF)
    return m, img


def model_and_img(cfg):
    return _model_and_img(_key(cfg))


def set_switch(switch, on):
    from glom_pytorch_amd import ops
    getattr(ops, switch)(on)


def both(switch, fn):
    """fn() with the switch on, then off; the switch is left on."""
    try:
        set_switch(switch, True)
        on = fn()
        set_switch(switch, False)
        off = fn()
    finally:
        set_switch(switch, True)
    torch.cuda.synchronize()
    return on, off


def forward_case(cfg, case):
    """Final levels and the return_all trajectory of one forward."""
    m, img = model_and_img(cfg)
    kw = dict(iters=ITERS)
    if case == "iters1":
        kw["iters"] = 1
    if case == "stateful":
        g = torch.Generator(device=DEV).manual_seed(3)
        n = (cfg["image_size"] // cfg["patch_size"]) ** 2
        kw["levels"] = torch.randn(2, n, cfg["levels"], cfg["dim"],
                                   device=DEV, generator=g).to(BF)
    if case == "levels2":
        m, img = model_and_img(dict(cfg, levels=2))
    if case == "graphs":
        m.enable_graphs()     # a fresh cache: captures with this setting
    try:
        with torch.no_grad():
            final = m(img, **kw).clone()
            traj = m(img, return_all=True, **kw).clone()
    finally:
        m.disable_graphs()
    torch.cuda.synchronize()
    assert torch.isfinite(final.float()).all()
    return final, traj


FORWARD_CASES = ["no_grad", "graphs", "stateful", "iters1", "levels2"]


def assert_forward_equal(switch, cfg, case):
    (f1, t1), (f0, t0) = both(switch, lambda: forward_case(cfg, case))
    assert torch.equal(f1, f0), case
    assert torch.equal(t1, t0), case
    assert torch.equal(t1[-1], f1), case


def grads(cfg, grad_iters, lmin, overlap_tail):
    """Trajectory and parameter gradients of one training step whose loss
    reads time grad_iters at the top level."""
    from glom_pytorch_amd.ops.functional import join_tail_stream
    m, img = model_and_img(cfg)
    m.zero_grad(set_to_none=True)
    traj = m(img, iters=ITERS, return_all=True, grad_iters=grad_iters,
             loss_level_min=lmin, overlap_tail=overlap_tail)
    traj[grad_iters][:, :, -1:].float().pow(2).sum().backward()
    if overlap_tail:
        join_tail_stream()
    torch.cuda.synchronize()
    g = {n: p.grad.clone() for n, p in m.named_parameters()
         if p.grad is not None}
    return traj.detach().clone(), g


def assert_grads_equal(switch, cfg, grad_iters, lmin, overlap_tail):
    (t1, g1), (t0, g0) = both(
        switch, lambda: grads(cfg, grad_iters, lmin, overlap_tail))
    assert torch.equal(t1, t0)
    assert set(g1) == set(g0) and len(g0) >= 10
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
    assert g0["bottom_up.net.1.weight"].float().abs().sum() > 0


def train(cfg, graph_step):
    from glom_pytorch_amd.parallel.trainer import DenoisingTrainer
    torch.manual_seed(0)
    m = Glom(**cfg).to(DEV, BF)
    tr = DenoisingTrainer(m, lr=1e-3, decode_step=4, graph_step=graph_step)
    s = cfg["image_size"]
    img = torch.randn(2, 3, s, s, device=DEV).to(BF)
    torch.manual_seed(1)
    losses = [tr.step(img, iters=ITERS) for _ in range(3)]
    torch.cuda.synchronize()
    return (losses, [q.detach().clone() for q in tr._params],
            [w.clone() for w in tr.master])


def assert_trainer_equal(switch, cfg, graph_step):
    (l1, p1, w1), (l0, p0, w0) = both(switch,
                                      lambda: train(cfg, graph_step))
    assert l1 == l0 and all(x == x for x in l1)
    assert len(p1) == len(p0) and len(w1) == len(w0) and len(w1) > 0
    for a, b in zip(p1 + w1, p0 + w0):
        assert torch.equal(a, b)
