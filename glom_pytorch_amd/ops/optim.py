"""Fused AdamW for bf16 training with fp32 master weights.

One HIP kernel pass per step (plus a two-stage deterministic grad-norm
reduction) replaces the per-step Python loop of: bf16->fp32 grad copies,
clip_grad_norm_, foreach-AdamW over the masters, and the fp32->bf16
parameter copy-back. Semantics match ``torch.optim.AdamW`` exactly
(decoupled weight decay, bias correction, the clip applied to grads before
the moment updates), and ``state_dict()`` mirrors torch's format so
checkpoints interchange with the plain-optimizer path.

hipGraph-replay-safe: the step counter lives in a device tensor that the
norm-finalize kernel increments, so a captured step() stays correct across
replays; ``steps_done()`` syncs the host mirror (one device read) before
checkpointing. The device counter is fp32 and exact up to 2^24 steps.

Per-param step caveat: torch increments a param's ``step`` only on steps
where it received a gradient; this class uses the global step count for
every present param's bias correction (params with ``grad=None`` are
skipped entirely, like torch). Identical whenever all params get grads
every step — the standard training path.

Two kernel paths with the same arithmetic (bit-identical for the same fp32
lr). The kernel-argument path (``k_adamw``) is used while there is no
schedule, every tensor has ``lr_scale == 1`` and the same weight decay, and
``lr`` has not been reassigned after construction. Otherwise the device-lr
path (``k_grad_norm_fin_sched`` + ``k_adamw_sched``) runs: ``lr`` is held in
a small device block next to the step counter, assigning ``opt.lr = x`` is a
stream-ordered fill of that block (no sync), and an ``LRSchedule`` is
evaluated on the device from the step counter every step, with no host
synchronisation, no allocation and the same three launches.

Hyperparameters under graph capture: on the kernel-argument path
``lr``/betas/eps/weight_decay are kernel arguments, so a captured step
bakes them in. The device-lr path is built so that ``lr`` and the schedule
stay live across replays (only betas, eps, ``max_grad_norm`` and the
per-tensor tables are kernel arguments there), but the trainer does not capture device-lr steps yet: it launches them
eagerly (see ``DenoisingTrainer``).
"""

from __future__ import annotations

import math

import torch

from glom_pytorch_amd.ops import _load_extension

_NPART = 1024   # must match OPT_NPART in native_ops.h

# device hyperparameter block layout: must match OPT_H_* in native_ops.h
_H_BASE_LR, _H_KIND, _H_WARMUP, _H_TOTAL, _H_MIN_RATIO, _H_LR_T = range(6)
_H_SIZE = 8


class LRSchedule:
    """Learning-rate factor as a function of the 0-based step index ``s``:
    linear warmup ``(s+1)/W`` for ``s < W``, then 1 (``constant``), a linear
    or a half-cosine decay from 1 at ``s = W`` to ``min_ratio`` at
    ``s = total_steps``, and ``min_ratio`` from there on. ``constant``
    ignores ``total_steps`` and ``min_ratio``.

    ``factor`` is the float64 specification; ``FusedAdamW`` evaluates the
    same formula in fp32 on the device."""

    KINDS = ("constant", "linear", "cosine")

    def __init__(self, kind: str = "constant", warmup_steps: int = 0,
                 total_steps: int = 0, min_ratio: float = 0.0):
        if kind not in self.KINDS:
            raise ValueError(f"kind must be one of {self.KINDS}, got {kind!r}")
        if int(warmup_steps) != warmup_steps or warmup_steps < 0:
            raise ValueError("warmup_steps must be an integer >= 0")
        if int(total_steps) != total_steps:
            raise ValueError("total_steps must be an integer")
        if kind != "constant" and not total_steps > warmup_steps:
            raise ValueError("total_steps must be > warmup_steps for a "
                             "decaying schedule")
        if not 0.0 <= min_ratio <= 1.0:
            raise ValueError("min_ratio must be in [0, 1]")
        self.kind = kind
        self.warmup_steps = int(warmup_steps)
        self.total_steps = int(total_steps)
        self.min_ratio = float(min_ratio)

    def factor(self, s: int) -> float:
        W, T, m = self.warmup_steps, self.total_steps, self.min_ratio
        if s < W:
            return (s + 1) / W
        if self.kind == "constant":
            return 1.0
        if s >= T:
            return m
        x = (s - W) / (T - W)
        if self.kind == "linear":
            return m + (1.0 - m) * (1.0 - x)
        return m + (1.0 - m) * 0.5 * (1.0 + math.cos(math.pi * x))

    def to_dict(self) -> dict:
        return {"kind": self.kind, "warmup_steps": self.warmup_steps,
                "total_steps": self.total_steps, "min_ratio": self.min_ratio}

    @classmethod
    def from_dict(cls, d: dict) -> "LRSchedule":
        return cls(d["kind"], d["warmup_steps"], d["total_steps"],
                   d["min_ratio"])

    def __eq__(self, other):
        return (isinstance(other, LRSchedule)
                and self.to_dict() == other.to_dict())

    def __repr__(self):
        return (f"LRSchedule({self.kind!r}, warmup_steps={self.warmup_steps},"
                f" total_steps={self.total_steps},"
                f" min_ratio={self.min_ratio})")


def _per_tensor(value, n: int, name: str) -> list[float]:
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError(f"{name}: expected {n} values, got {len(value)}")
        return [float(v) for v in value]
    return [float(value)] * n


class FusedAdamW:
    def __init__(self, params: list[torch.Tensor],
                 masters: list[torch.Tensor], *, lr: float = 1e-3,
                 betas: tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay=1e-2,
                 max_grad_norm: float = 0.0, lr_scale=1.0,
                 schedule: LRSchedule | None = None):
        """``weight_decay`` and ``lr_scale`` take a float or one value per
        parameter; ``schedule`` an ``LRSchedule`` or None (constant lr)."""
        assert len(params) == len(masters)
        self.params = list(params)
        self.masters = list(masters)
        self.betas = betas
        self.eps = eps
        self.max_grad_norm = max_grad_norm
        n = len(self.params)
        self._wd = _per_tensor(weight_decay, n, "weight_decay")
        self._lr_scale = _per_tensor(lr_scale, n, "lr_scale")
        dev = masters[0].device
        self.exp_avg = [torch.zeros_like(m) for m in masters]
        self.exp_avg_sq = [torch.zeros_like(m) for m in masters]
        self._partials = torch.zeros(_NPART, dtype=torch.float32, device=dev)
        self._norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self._step_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self._step_host = 0      # mirror; device tensor is authoritative
        # base lr, schedule parameters and the per-step lr_t output
        self._hyper = torch.zeros(_H_SIZE, dtype=torch.float32, device=dev)
        self._lr = float(lr)
        self._lr_assigned = False   # lr reassigned after construction
        self._lr_t_live = False     # last step went through the device block
        self._schedule = schedule
        self._write_hyper()

    # ------------------------- hyperparameters ------------------------ #

    @property
    def lr(self) -> float:
        """Base learning rate. Assigning it writes the device block with a
        stream-ordered fill (no sync): the next step, captured or not, uses
        it."""
        return self._lr

    @lr.setter
    def lr(self, value: float):
        self._lr = float(value)
        self._lr_assigned = True
        self._hyper[_H_BASE_LR:_H_BASE_LR + 1].fill_(self._lr)

    @property
    def schedule(self) -> LRSchedule | None:
        return self._schedule

    @schedule.setter
    def schedule(self, value: LRSchedule | None):
        self._schedule = value
        self._write_hyper()

    @property
    def weight_decay(self):
        """The weight decay: a float while every tensor shares one value,
        else the per-parameter list."""
        if all(w == self._wd[0] for w in self._wd):
            return self._wd[0]
        return list(self._wd)

    @weight_decay.setter
    def weight_decay(self, value):
        self._wd = _per_tensor(value, len(self.params), "weight_decay")

    @property
    def lr_scale(self):
        if all(v == self._lr_scale[0] for v in self._lr_scale):
            return self._lr_scale[0]
        return list(self._lr_scale)

    @lr_scale.setter
    def lr_scale(self, value):
        self._lr_scale = _per_tensor(value, len(self.params), "lr_scale")

    def _write_hyper(self):
        sc = self._schedule
        f0 = sc.factor(0) if sc is not None else 1.0
        host = torch.zeros(_H_SIZE, dtype=torch.float32)
        host[_H_BASE_LR] = self._lr
        if sc is not None:
            host[_H_KIND] = LRSchedule.KINDS.index(sc.kind)
            host[_H_WARMUP] = sc.warmup_steps
            host[_H_TOTAL] = sc.total_steps
            host[_H_MIN_RATIO] = sc.min_ratio
        host[_H_LR_T] = self._lr * f0
        self._hyper.copy_(host)

    def _uses_device_lr(self) -> bool:
        return (self._schedule is not None or self._lr_assigned
                or any(v != 1.0 for v in self._lr_scale)
                or any(w != self._wd[0] for w in self._wd))

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            p.grad = None

    @torch.no_grad()
    def step(self):
        ext = _load_extension()
        gs, mws, m1s, m2s, pws, scales, wds = [], [], [], [], [], [], []
        for i, p in enumerate(self.params):
            if p.grad is None:
                continue
            gs.append(p.grad)
            mws.append(self.masters[i])
            m1s.append(self.exp_avg[i])
            m2s.append(self.exp_avg_sq[i])
            pws.append(p.data)
            scales.append(self._lr_scale[i])
            wds.append(self._wd[i])
        if not gs:
            return
        if self._uses_device_lr():
            ext.fused_adamw_sched(gs, mws, m1s, m2s, pws, scales, wds,
                                  self.betas[0], self.betas[1], self.eps,
                                  self.max_grad_norm, self._partials,
                                  self._norm, self._step_dev, self._hyper)
            self._lr_t_live = True
        else:
            ext.fused_adamw(gs, mws, m1s, m2s, pws, self._lr, self.betas[0],
                            self.betas[1], self.eps, self._wd[0],
                            self.max_grad_norm, self._partials, self._norm,
                            self._step_dev)
            self._lr_t_live = False
        self._step_host += 1

    def note_replays(self, n: int):
        """Called by graph-replay drivers: n captured steps ran without
        Python; keep the host mirror roughly in sync (device is exact)."""
        self._step_host += n

    def steps_done(self) -> int:
        """Exact step count (reads the device counter; syncs)."""
        return int(self._step_dev.item())

    def current_lr(self) -> float:
        """The base-group lr the most recent step used (``lr * factor``;
        per-tensor ``lr_scale`` comes on top). Reads the device block (one
        sync) when that step went through it."""
        if self._lr_t_live:
            return float(self._hyper[_H_LR_T].item())
        return self._lr

    # ----------------- torch.optim.AdamW state_dict parity -------------

    def _groups(self) -> list[list[int]]:
        """Parameter indices partitioned by distinct (lr_scale, wd), in
        order of first appearance."""
        groups: dict = {}
        for i in range(len(self.params)):
            groups.setdefault((self._lr_scale[i], self._wd[i]), []).append(i)
        return list(groups.values())

    def state_dict(self):
        step = float(self.steps_done())
        state = {}
        for i in range(len(self.params)):
            state[i] = {
                "step": torch.tensor(step),
                "exp_avg": self.exp_avg[i],
                "exp_avg_sq": self.exp_avg_sq[i],
            }
        # torch numbers params consecutively across groups
        order = [i for idx in self._groups() for i in idx]
        pos = {i: k for k, i in enumerate(order)}
        state = {pos[i]: st for i, st in state.items()}
        groups = []
        for idx in self._groups():
            groups.append({
                "lr": self._lr * self._lr_scale[idx[0]],
                "betas": tuple(self.betas), "eps": self.eps,
                "weight_decay": self._wd[idx[0]], "amsgrad": False,
                "foreach": None, "maximize": False, "capturable": False,
                "differentiable": False, "fused": None,
                "params": [pos[i] for i in idx],
            })
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        # format-only use on an instance built without __init__ (no device):
        # one default group, no device block to refresh
        n = len(self.masters)
        if not hasattr(self, "_lr_scale"):
            self._lr_scale, self._wd = [1.0] * n, [0.0] * n
        mine = self._groups()
        if len(groups) != len(mine) or any(
                len(g["params"]) != len(idx) for g, idx in zip(groups, mine)):
            raise ValueError("loaded state dict's parameter groups do not "
                             "match this optimizer's (lr_scale, "
                             "weight_decay) partition")
        g0 = groups[0]
        self.betas = tuple(g0["betas"])
        self.eps = g0["eps"]
        for g, idx in zip(groups, mine):
            for i in idx:
                self._wd[i] = float(g["weight_decay"])
        # group lr = base lr * lr_scale; lr_scale stays the constructor's
        s0 = self._lr_scale[mine[0][0]]
        if s0 != 0.0:
            self._lr = float(g0["lr"]) / s0
        if hasattr(self, "_hyper"):
            self._write_hyper()
        order = [i for idx in mine for i in idx]
        step = 0.0
        for k, i in enumerate(order):
            m = self.masters[i]
            st = sd["state"].get(k, sd["state"].get(str(k)))
            if st is None:
                continue
            self.exp_avg[i].copy_(st["exp_avg"].to(m.device,
                                                   torch.float32))
            self.exp_avg_sq[i].copy_(st["exp_avg_sq"].to(m.device,
                                                         torch.float32))
            s = st["step"]
            step = float(s.item() if torch.is_tensor(s) else s)
        self._step_dev.fill_(step)
        self._step_host = int(step)
