"""Learning-rate schedules and no-decay parameter groups on the torch-AdamW
(CPU) trainer path: the ``LRSchedule`` specification, the per-step group lr,
the two weight-decay groups and a mid-schedule checkpoint round trip."""

import math

import pytest
import torch

from conftest import SMALL, SMALL_BATCH, SMALL_ITERS
from glom_pytorch_amd import Glom
from glom_pytorch_amd.ops.optim import LRSchedule
from glom_pytorch_amd.parallel.trainer import DenoisingTrainer

KINDS = ("constant", "linear", "cosine")


# ----------------------------- LRSchedule ------------------------------ #

@pytest.mark.parametrize("kind", KINDS)
def test_factor_warmup_plateau_and_floor(kind):
    W, T, m = 5, 12, 0.1
    sc = LRSchedule(kind, warmup_steps=W, total_steps=T, min_ratio=m)
    for s in range(W):
        assert sc.factor(s) == (s + 1) / W
    assert sc.factor(W) == 1.0
    for s in (T, T + 1, T + 100):
        assert sc.factor(s) == (1.0 if kind == "constant" else m)
    fs = [sc.factor(s) for s in range(W, T + 1)]
    assert all(a >= b for a, b in zip(fs, fs[1:])), fs
    assert all(m <= f <= 1.0 for f in fs)


def test_factor_formulas():
    lin = LRSchedule("linear", warmup_steps=2, total_steps=10, min_ratio=0.2)
    cos = LRSchedule("cosine", warmup_steps=2, total_steps=10, min_ratio=0.2)
    for s in range(2, 10):
        x = (s - 2) / 8
        assert lin.factor(s) == pytest.approx(0.2 + 0.8 * (1 - x), abs=1e-15)
        assert cos.factor(s) == pytest.approx(
            0.2 + 0.8 * 0.5 * (1 + math.cos(math.pi * x)), abs=1e-15)
    # no warmup: the first step already runs at the full rate
    assert LRSchedule("cosine", 0, 4).factor(0) == 1.0
    assert LRSchedule("constant").factor(0) == 1.0
    assert LRSchedule("constant").factor(10 ** 6) == 1.0


@pytest.mark.parametrize("kwargs", [
    dict(kind="exponential", total_steps=10),
    dict(kind="cosine", warmup_steps=-1, total_steps=10),
    dict(kind="cosine", warmup_steps=5, total_steps=5),
    dict(kind="linear", warmup_steps=5, total_steps=3),
    dict(kind="linear", warmup_steps=0, total_steps=0),
    dict(kind="cosine", total_steps=10, min_ratio=-0.1),
    dict(kind="cosine", total_steps=10, min_ratio=1.5),
    dict(kind="constant", warmup_steps=2.5),
])
def test_invalid_arguments_raise(kwargs):
    with pytest.raises(ValueError):
        LRSchedule(**kwargs)


def test_dict_round_trip():
    sc = LRSchedule("cosine", warmup_steps=3, total_steps=9, min_ratio=0.25)
    back = LRSchedule.from_dict(sc.to_dict())
    assert back == sc
    assert [back.factor(s) for s in range(12)] == \
        [sc.factor(s) for s in range(12)]


# ------------------------------- trainer ------------------------------- #

def _trainer(seed=0, **kw):
    torch.manual_seed(seed)
    return DenoisingTrainer(Glom(**SMALL), lr=1e-3, noise_std=0.5, **kw)


def _img(seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(SMALL_BATCH, 3, SMALL["image_size"],
                       SMALL["image_size"], generator=g)


def test_trainer_cosine_schedule_sets_group_lr():
    sc = LRSchedule("cosine", warmup_steps=3, total_steps=6, min_ratio=0.1)
    tr = _trainer(lr_schedule=sc, no_decay=True)
    img = _img()
    for k in range(8):
        tr.step(img, iters=SMALL_ITERS)
        want = 1e-3 * sc.factor(k)
        for g in tr.opt.param_groups:
            assert g["lr"] == want, (k, g["lr"], want)
        assert tr.current_lr() == want


def test_default_is_one_group_constant_lr():
    tr = _trainer()
    assert len(tr.opt.param_groups) == 1
    assert tr.opt.param_groups[0]["weight_decay"] == 1e-2
    assert tr.current_lr() == 1e-3
    tr.step(_img(), iters=SMALL_ITERS)
    assert tr.opt.param_groups[0]["lr"] == 1e-3
    assert tr.current_lr() == 1e-3


def test_no_decay_groups():
    tr = _trainer(no_decay=True)
    assert len(tr.opt.param_groups) == 2
    named = (list(tr.model.named_parameters())
             + [("decoder." + n, p)
                for n, p in tr.decoder.named_parameters()])
    want_zero = {n for n, p in named
                 if p.ndim <= 1 or n in ("pos_emb.weight", "init_levels")}
    # sanity: the rule is not vacuous either way
    assert {"pos_emb.weight", "init_levels", "bottom_up.net.1.bias",
            "decoder.0.bias"} <= want_zero
    assert "bottom_up.net.1.weight" not in want_zero
    by_id = {id(p): n for n, p in named}
    seen = set()
    for g in tr.opt.param_groups:
        names = {by_id[id(p)] for p in g["params"]}
        seen |= names
        if g["weight_decay"] == 0.0:
            assert names == want_zero
        else:
            assert g["weight_decay"] == 1e-2
            assert names == set(by_id.values()) - want_zero
    assert seen == set(by_id.values())
    assert sorted(g["weight_decay"] for g in tr.opt.param_groups) \
        == [0.0, 1e-2]


def test_checkpoint_round_trip_mid_schedule(tmp_path):
    sc = LRSchedule("cosine", warmup_steps=2, total_steps=5, min_ratio=0.1)
    img = _img()
    path = str(tmp_path / "ck.pt")

    ta = _trainer(lr_schedule=sc, no_decay=True)
    for _ in range(3):
        ta.step(img, iters=SMALL_ITERS)
    ta.save_checkpoint(path)
    lrs_a = []
    for _ in range(3):
        ta.step(img, iters=SMALL_ITERS)
        lrs_a.append(ta.current_lr())
    assert lrs_a == [1e-3 * sc.factor(k) for k in (3, 4, 5)]

    # a fresh trainer (other init, no schedule of its own) takes weights,
    # step count, schedule and RNG from the checkpoint
    tb = _trainer(seed=7, no_decay=True)
    tb.load_checkpoint(path)
    assert tb.lr_schedule == sc
    lrs_b = []
    for _ in range(3):
        tb.step(img, iters=SMALL_ITERS)
        lrs_b.append(tb.current_lr())
    assert lrs_b == lrs_a
    for (n, pa), (_, pb) in zip(ta.model.named_parameters(),
                                tb.model.named_parameters()):
        assert torch.equal(pa, pb), n
    for pa, pb in zip(ta.decoder.parameters(), tb.decoder.parameters()):
        assert torch.equal(pa, pb)

    with pytest.raises(ValueError):
        _trainer(no_decay=False).load_checkpoint(path)
