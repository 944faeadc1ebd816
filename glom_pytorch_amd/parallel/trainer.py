"""Denoising self-supervised trainer for GLOM (the reference's training
recipe, README.md:56-90): noise the image, run the model with return_all,
decode the top level at a mid-iteration timestep back to pixels, MSE against
the clean image. Adds what the reference leaves to the user: optimizer,
data-parallel gradient sync, checkpointing, metrics — and, on the native
GPU path, hipGraph capture of the ENTIRE training step (noise + forward +
backward + fused AdamW), replayed as a single graph launch per step."""

from __future__ import annotations

import json
import os
import time
import warnings

import torch
import torch.distributed as dist
import torch.nn.functional as F
from einops.layers.torch import Rearrange
from torch import nn

from glom_pytorch_amd.parallel.ddp import BucketedDDP
from glom_pytorch_amd.parallel.failure import Heartbeat
from glom_pytorch_amd.ops.functional import trajectory_at


class _DecoderLinear(nn.Linear):
    """nn.Linear whose bf16 GPU bias gradient comes from the native
    fixed-order column sum (run-to-run reproducible); everything else, and
    every other device/dtype, is the stock layer."""

    def forward(self, x):
        if (x.is_cuda and x.dtype == torch.bfloat16
                and self.bias is not None and torch.is_grad_enabled()):
            from glom_pytorch_amd.ops.functional import LinearFixedBiasGradFn
            return LinearFixedBiasGradFn.apply(x, self.weight, self.bias)
        return super().forward(x)


class DenoisingDecoder(nn.Sequential):
    """Top-level embedding -> image patches (README.md:78-81)."""

    def __init__(self, dim: int, image_size: int, patch_size: int):
        side = image_size // patch_size
        super().__init__(
            _DecoderLinear(dim, patch_size ** 2 * 3),
            Rearrange("b (h w) (p1 p2 c) -> b c (h p1) (w p2)",
                      h=side, w=side, p1=patch_size, p2=patch_size),
        )


class DenoisingTrainer:
    def __init__(self, model, *, lr=3e-4, noise_std=1.0, decode_step=7,
                 grad_clip=1.0, distributed=False, bucket_bytes=16 << 20,
                 process_group=None, graph_step=True, overlap_tail=True,
                 micro_batches=1, log_path=None, contrast_weight=0.0,
                 contrast_level=-1, contrast_temperature=0.1,
                 contrast_negatives="other_images", level_cone=True,
                 lr_schedule=None, no_decay=False):
        """``process_group``: the group whose ranks are data-parallel
        replicas (default: the global group). For 2-D DP x SP meshes pass
        the DP subgroup here — BucketedDDP AVERAGES over its group, which
        is correct for DP replicas; SP shards need a separate SUM
        all-reduce over the SP subgroup (see parallel/sequence.py).

        ``graph_step``: hipGraph-capture the whole training step on the
        native bf16 GPU path (keyed on batch shape + iters) and replay it;
        falls back to eager launches automatically if capture fails.
        Disable with graph_step=False or GLOM_NO_GRAPH_STEP=1.

        ``contrast_weight`` (default 0.0 = the plain denoising step, launch
        for launch): when > 0 every step noises the batch twice, runs ONE
        forward on the 2B concatenation, averages the denoising loss over
        both views and adds ``contrast_weight *
        column_contrastive_loss(top_a, top_b)`` between the two views'
        level ``contrast_level`` at the decode step
        (``glom_pytorch_amd.contrast``; ``contrast_temperature`` and
        ``contrast_negatives`` are passed through). The settings are
        constructor constants, so captured graphs stay keyed on batch shape
        and iters. Micro-batching with the term on is not implemented
        (negatives would have to cross chunks): ``step`` raises
        ``NotImplementedError``.

        ``level_cone``: pass the model the lowest level the loss reads
        (``loss_level_min``: the top level, or ``contrast_level`` when the
        contrastive term is on and lower), so the backward skips the level
        groups whose gradient is exactly zero. Same losses and updates.
        Disable with level_cone=False or GLOM_NO_LEVEL_CONE=1.

        ``lr_schedule`` (default None = constant ``lr``): an
        ``ops.optim.LRSchedule``; step ``k`` (0-based) runs at
        ``lr * lr_schedule.factor(k)``. The fused optimizer evaluates it on
        the device from its step counter (no host sync, no extra launch);
        the torch-AdamW paths set their groups' lr from the same formula
        before each step.

        ``no_decay`` (default False = weight decay 1e-2 everywhere): weight
        decay 0 for every parameter with ``ndim <= 1`` plus
        ``pos_emb.weight`` and ``init_levels``.

        With a schedule, ``no_decay``, or once ``trainer.opt.lr`` is
        assigned on the fused path, the step is launched eagerly instead of
        replayed from the captured graph (whose kernel arguments are
        frozen): the assignment takes effect on the next step, at the
        eager-launch step cost. Capturing such steps is not implemented."""
        from glom_pytorch_amd.contrast import NEGATIVES
        from glom_pytorch_amd.ops.optim import LRSchedule
        if lr_schedule is not None and not isinstance(lr_schedule,
                                                      LRSchedule):
            raise ValueError("lr_schedule must be an LRSchedule or None")
        self.base_lr = float(lr)
        self.lr_schedule = lr_schedule
        self.no_decay = bool(no_decay)
        if contrast_weight < 0 or not contrast_temperature > 0:
            raise ValueError("contrast_weight must be >= 0 and "
                             "contrast_temperature > 0")
        if contrast_negatives not in NEGATIVES:
            raise ValueError(f"contrast_negatives must be one of {NEGATIVES}")
        self.contrast_weight = float(contrast_weight)
        self.contrast_level = int(contrast_level)
        self.contrast_temperature = float(contrast_temperature)
        self.contrast_negatives = contrast_negatives
        self.model = model
        self.dim = model.dim
        self.decode_step = decode_step
        self.noise_std = noise_std
        p = next(model.parameters())
        self.decoder = DenoisingDecoder(
            model.dim, model.image_size, model.patch_size
        ).to(p.device, p.dtype)
        self.distributed = distributed and dist.is_initialized()
        self.ddp_model = self.ddp_dec = self.heartbeat = None
        if self.distributed:
            self.ddp_model = BucketedDDP(model, bucket_bytes,
                                         process_group=process_group)
            self.ddp_dec = BucketedDDP(self.decoder, bucket_bytes,
                                       process_group=process_group)
            # rank-liveness probe: a hung peer becomes a clean abort
            self.heartbeat = Heartbeat(every_steps=50)
        params = list(model.parameters()) + list(self.decoder.parameters())
        self._params = params
        names = ([n for n, _ in model.named_parameters()]
                 + ["decoder." + n
                    for n, _ in self.decoder.named_parameters()])
        # per-parameter weight decay: with no_decay, none on biases and
        # other <=1-D tensors nor on the two embedding tables
        wds = [0.0 if self.no_decay and (
                   q.ndim <= 1 or n in ("pos_emb.weight", "init_levels"))
               else 1e-2 for n, q in zip(names, params)]

        def torch_adamw(tensors):
            if not self.no_decay:
                return torch.optim.AdamW(tensors, lr=lr, foreach=True)
            # groups in order of first appearance, as FusedAdamW
            # partitions them, so optimizer states interchange
            groups: dict = {}
            for t, w in zip(tensors, wds):
                groups.setdefault(w, []).append(t)
            return torch.optim.AdamW(
                [{"params": ts, "weight_decay": w}
                 for w, ts in groups.items()], lr=lr, foreach=True)
        # bf16 training keeps fp32 master weights: updates of size lr*grad
        # would otherwise partially round away in bf16 parameter storage
        self.master = None
        self.fused_opt = None
        if p.dtype == torch.bfloat16:
            self.master = [q.detach().float().requires_grad_(False)
                           for q in params]
            if p.is_cuda and self._ops_available():
                # single-kernel AdamW: bf16 grads -> fp32 m/v/master ->
                # bf16 params, with the global-norm clip fused
                from glom_pytorch_amd.ops.optim import FusedAdamW
                self.fused_opt = FusedAdamW(
                    params, self.master, lr=lr,
                    weight_decay=wds if self.no_decay else 1e-2,
                    max_grad_norm=grad_clip if grad_clip else 0.0,
                    schedule=lr_schedule)
                self.opt = self.fused_opt
            else:
                self.opt = torch_adamw(self.master)
        else:
            self.opt = torch_adamw(params)
        self.grad_clip = grad_clip
        self.step_idx = 0
        self.log_path = log_path
        self.graph_step = (graph_step
                           and os.environ.get("GLOM_NO_GRAPH_STEP", "0")
                           != "1")
        self.level_cone = (level_cone
                           and os.environ.get("GLOM_NO_LEVEL_CONE", "0")
                           != "1")
        self.overlap_tail = (overlap_tail
                             and os.environ.get("GLOM_NO_OVERLAP_TAIL",
                                                "0") != "1")
        # pipelined microbatching: split the batch in `micro_batches`
        # chunks; each chunk's loss is scaled 1/m so the summed grads
        # equal the full-batch gradient EXACTLY (mean-MSE is linear in
        # batch averaging); chunk i+1's forward runs on a side stream
        # overlapping chunk i's backward.
        self.micro_batches = int(os.environ.get("GLOM_MICRO_BATCHES",
                                                str(micro_batches)))
        self._micro_stream = None
        self._graphs: dict = {}

    def _loss_level_min(self, contrast: bool = False):
        """Lowest level the step's loss reads at the decode step, or None
        with the level cone off."""
        if not self.level_cone:
            return None
        L = self.model.levels
        return min(L - 1, self.contrast_level % L) if contrast else L - 1

    @staticmethod
    def _ops_available():
        from glom_pytorch_amd import ops
        return ops.available()

    def _torch_opt_step(self):
        """Step of the torch-AdamW paths (CPU, fp32, no extension). With a
        schedule, every group first gets ``base * factor(step_idx)``: the
        specification the fused optimizer evaluates on the device."""
        if self.lr_schedule is not None:
            lr = self.base_lr * self.lr_schedule.factor(self.step_idx)
            for g in self.opt.param_groups:
                g["lr"] = lr
        self.opt.step()

    def current_lr(self) -> float:
        """The learning rate the most recent step used (the base lr before
        the first). One host sync on the fused path."""
        if self.fused_opt is not None:
            return self.fused_opt.current_lr()
        return float(self.opt.param_groups[0]["lr"])

    # ------------------------------ stepping -------------------------- #

    def step(self, img: torch.Tensor, iters: int | None = None,
             sync_loss: bool = True):
        """One denoising training step. With sync_loss=False the loss is
        returned as a device tensor (no host sync), letting the host run
        ahead and queue the next step's launches."""
        iters = iters if iters is not None else 2 * self.model.levels
        if self._graph_usable(img):
            loss = self._graphed_step(img, iters)
        else:
            loss = self._eager_step(img, iters)
        self.step_idx += 1
        if self.heartbeat is not None:
            self.heartbeat.tick()
        return loss.item() if sync_loss else loss.detach()

    def _graph_usable(self, img) -> bool:
        # micro-pipelining accumulates grads across streams; the
        # AccumulateGrad node's stream mismatch breaks hipGraph capture
        # (torch warns, replay faults) — micro mode runs eager-launched
        # a captured step bakes in the optimizer's kernel-argument lr; once
        # lr lives in device memory (schedule, per-tensor groups, or an lr
        # assigned after construction) steps are launched eagerly, where it
        # is live. Capturing those steps is left out for now.
        return (self.graph_step and self.micro_batches == 1
                and self.fused_opt is not None
                and not self.fused_opt._uses_device_lr()
                and img.is_cuda and img.dtype == torch.bfloat16
                and not getattr(self.model, "force_eager", False)
                and os.environ.get("GLOM_FORCE_EAGER", "0") != "1")

    def _eager_step(self, img: torch.Tensor, iters: int) -> torch.Tensor:
        if self.contrast_weight > 0:
            return self._contrast_step(img, iters)
        m = self.micro_batches
        if (m > 1 and img.is_cuda and img.shape[0] % m == 0
                and not getattr(self.model, "force_eager", False)):
            return self._micro_step(img, iters, m)
        t = min(self.decode_step, iters)
        self.opt.zero_grad(set_to_none=True)
        noised = img + torch.randn_like(img) * self.noise_std
        # the loss reads only trajectory time t: iterations >= t carry
        # exactly-zero gradient, so they run forward-only (grad_iters) —
        # identical values and gradients, ~(iters-t)/iters less backward.
        # overlap_tail additionally runs them on a side stream so they
        # overlap the backward below; join_tail_stream() before the
        # optimizer guarantees no weight write races the tail's reads.
        overlap = (self.overlap_tail and img.is_cuda
                   and not getattr(self.model, "force_eager", False))
        all_levels = self.model(noised, iters=iters, return_all=True,
                                grad_iters=t, overlap_tail=overlap,
                                loss_level_min=self._loss_level_min())
        top = trajectory_at(all_levels, t)[:, :, -1]
        recon = self.decoder(top)
        loss = F.mse_loss(recon.float(), img.float())
        loss.backward()
        if self.distributed:
            self.ddp_model.finalize()
            self.ddp_dec.finalize()
        if overlap:
            from glom_pytorch_amd.ops.functional import join_tail_stream
            join_tail_stream()
        if self.fused_opt is not None:
            self.fused_opt.step()
        elif self.master is not None:
            with torch.no_grad():
                for mw, q in zip(self.master, self._params):
                    # None (not stale) when the param got no grad this
                    # step, e.g. init_levels on the stateful path
                    mw.grad = q.grad.float() if q.grad is not None else None
                if self.grad_clip:
                    torch.nn.utils.clip_grad_norm_(self.master,
                                                   self.grad_clip)
                self._torch_opt_step()
                for mw, q in zip(self.master, self._params):
                    q.data.copy_(mw)
        else:
            if self.grad_clip:
                torch.nn.utils.clip_grad_norm_(
                    [q for g in self.opt.param_groups for q in g["params"]],
                    self.grad_clip)
            self._torch_opt_step()
        return loss.detach()

    def _contrast_step(self, img: torch.Tensor, iters: int) -> torch.Tensor:
        """Denoising step over two independently noised views of the batch
        (one 2B forward) plus the weighted column-contrastive term between
        the views. Both losses read trajectory time t only, so grad_iters
        and the overlapped tail stay valid as in ``_eager_step``."""
        from glom_pytorch_amd.contrast import column_contrastive_loss
        if self.micro_batches > 1:
            raise NotImplementedError(
                "contrast_weight > 0 does not support micro_batches > 1")
        t = min(self.decode_step, iters)
        B = img.shape[0]
        self.opt.zero_grad(set_to_none=True)
        noised = torch.cat(
            (img + torch.randn_like(img) * self.noise_std,
             img + torch.randn_like(img) * self.noise_std))
        overlap = (self.overlap_tail and img.is_cuda
                   and not getattr(self.model, "force_eager", False))
        all_levels = self.model(noised, iters=iters, return_all=True,
                                grad_iters=t, overlap_tail=overlap,
                                loss_level_min=self._loss_level_min(True))
        at_t = trajectory_at(all_levels, t)
        recon = self.decoder(at_t[:, :, -1])
        clean = torch.cat((img, img))
        loss = F.mse_loss(recon.float(), clean.float())
        lvl = at_t[:, :, self.contrast_level]
        loss = loss + self.contrast_weight * column_contrastive_loss(
            lvl[:B], lvl[B:], temperature=self.contrast_temperature,
            negatives=self.contrast_negatives)
        loss.backward()
        if self.distributed:
            self.ddp_model.finalize()
            self.ddp_dec.finalize()
        if overlap:
            from glom_pytorch_amd.ops.functional import join_tail_stream
            join_tail_stream()
        if self.fused_opt is not None:
            self.fused_opt.step()
        elif self.master is not None:
            with torch.no_grad():
                for mw, q in zip(self.master, self._params):
                    mw.grad = q.grad.float() if q.grad is not None else None
                if self.grad_clip:
                    torch.nn.utils.clip_grad_norm_(self.master,
                                                   self.grad_clip)
                self._torch_opt_step()
                for mw, q in zip(self.master, self._params):
                    q.data.copy_(mw)
        else:
            if self.grad_clip:
                torch.nn.utils.clip_grad_norm_(
                    [q for g in self.opt.param_groups for q in g["params"]],
                    self.grad_clip)
            self._torch_opt_step()
        return loss.detach()

    def _micro_forward(self, half: torch.Tensor, iters: int, t: int,
                       scale: float) -> torch.Tensor:
        noised = half + torch.randn_like(half) * self.noise_std
        traj = self.model(noised, iters=iters, return_all=True,
                          grad_iters=t, overlap_tail=True,
                          loss_level_min=self._loss_level_min())
        recon = self.decoder(trajectory_at(traj, t)[:, :, -1])
        return F.mse_loss(recon.float(), half.float()) * scale

    def _micro_step(self, img: torch.Tensor, iters: int,
                    m: int) -> torch.Tensor:
        """Pipelined microbatches: forward of chunk i+1 (on a side
        stream) overlaps backward of chunk i. Gradients are EXACTLY the
        full-batch gradient: mean-MSE over the batch = (1/m) sum of the
        chunk means, and autograd sums the scaled chunk grads."""
        t = min(self.decode_step, iters)
        self.opt.zero_grad(set_to_none=True)
        if self._micro_stream is None:
            self._micro_stream = torch.cuda.Stream()
        s_f = self._micro_stream
        halves = img.chunk(m)
        if self.distributed:
            self.ddp_model.set_accumulate(True)
            self.ddp_dec.set_accumulate(True)
        cur = torch.cuda.current_stream()
        losses = []
        pending = self._micro_forward(halves[0], iters, t, 1.0 / m)
        for i in range(1, m):
            # fork chunk i's forward before launching chunk i-1's backward
            ev = torch.cuda.Event()
            ev.record(cur)
            with torch.cuda.stream(s_f):
                s_f.wait_event(ev)
                nxt = self._micro_forward(halves[i], iters, t, 1.0 / m)
            pending.backward()
            losses.append(pending.detach())
            if self.distributed and i == m - 1:
                self.ddp_model.set_accumulate(False)
                self.ddp_dec.set_accumulate(False)
                # counts were consumed? hooks were suppressed: reset
                self.ddp_model._reset_counts()
                self.ddp_dec._reset_counts()
            pending = nxt
        pending.backward()   # engine runs this chunk's ops on s_f
        losses.append(pending.detach())
        cur.wait_stream(s_f)
        if self.distributed:
            self.ddp_model.finalize()
            self.ddp_dec.finalize()
        from glom_pytorch_amd.ops.functional import join_tail_stream
        join_tail_stream()
        loss = losses[0]
        for l in losses[1:]:
            loss = loss + l
        if self.fused_opt is not None:
            self.fused_opt.step()
        elif self.master is not None:
            with torch.no_grad():
                for mw, q in zip(self.master, self._params):
                    mw.grad = (q.grad.float() if q.grad is not None
                               else None)
                if self.grad_clip:
                    torch.nn.utils.clip_grad_norm_(self.master,
                                                   self.grad_clip)
                self._torch_opt_step()
                for mw, q in zip(self.master, self._params):
                    q.data.copy_(mw)
        else:
            self._torch_opt_step()
        return loss.detach()

    # --------------------- hipGraph-captured step --------------------- #

    def _graphed_step(self, img: torch.Tensor, iters: int) -> torch.Tensor:
        key = (tuple(img.shape), iters)
        entry = self._graphs.get(key)
        if entry is None:
            entry = self._capture(img, iters)
            self._graphs[key] = entry
        if entry is False:
            return self._eager_step(img, iters)
        entry["img"].copy_(img)
        entry["graph"].replay()
        self.fused_opt.note_replays(1)
        return entry["loss"]

    def _capture(self, img: torch.Tensor, iters: int):
        """Record noise + forward (all `iters` GLOM steps) + backward +
        bucketed all-reduce (if distributed) + fused AdamW as ONE hipGraph.
        torch.cuda.graph handles the philox RNG state, so every replay
        draws fresh noise. Any capture failure falls back to eager."""
        if self.distributed and os.environ.get("GLOM_GRAPH_DIST",
                                               "1") == "0":
            return False
        try:
            static_img = img.clone()
            # snapshot optimizer/weight state: the warmup steps below are
            # real updates, rolled back so a graphed step == one step
            fo = self.fused_opt
            with torch.no_grad():
                snap = ([m.clone() for m in self.master]
                        + [t.clone() for t in fo.exp_avg]
                        + [t.clone() for t in fo.exp_avg_sq]
                        + [q.detach().clone() for q in self._params]
                        + [fo._step_dev.clone()])
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):     # allocator/runtime warmup
                    self._eager_step(static_img, iters)
            torch.cuda.current_stream().wait_stream(s)
            with torch.no_grad():
                live = (self.master + fo.exp_avg + fo.exp_avg_sq
                        + [q.data for q in self._params] + [fo._step_dev])
                for dst, src in zip(live, snap):
                    dst.copy_(src)
                fo._step_host = max(0, fo._step_host - 2)
            # start from grads=None: backward inside capture then ASSIGNS
            # fresh graph-pool grad tensors (no accumulate node recorded)
            for q in self._params:
                q.grad = None
            graph = torch.cuda.CUDAGraph()
            # (a) flush pending destructors NOW and keep the cyclic GC off
            # during capture: a stale CUDAGraph/tensor destructor firing
            # mid-capture makes HIP API calls that invalidate the capture
            # (the replay then segfaults); (b) thread_local error mode:
            # the RCCL watchdog thread polls events on this device during
            # capture and must not invalidate it either.
            import gc
            gc.collect()
            gc_was_enabled = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(graph,
                                      capture_error_mode="thread_local"):
                    loss = self._eager_step(static_img, iters)
            finally:
                if gc_was_enabled:
                    gc.enable()
            # capture RECORDS the step without executing it: undo the
            # Python-side count bump from the captured call
            fo._step_host = max(0, fo._step_host - 1)
            return {"graph": graph, "img": static_img, "loss": loss}
        except Exception as e:  # pragma: no cover - GPU/runtime specific
            warnings.warn(f"training-step hipGraph capture failed "
                          f"({type(e).__name__}: {e}); using eager "
                          f"launches")
            return False

    def log(self, **metrics):
        if self.log_path:
            with open(self.log_path, "a") as f:
                f.write(json.dumps({"step": self.step_idx,
                                    "time": time.time(), **metrics}) + "\n")

    # -------------------- checkpoint / resume --------------------

    def save_checkpoint(self, path: str):
        if self.distributed and dist.get_rank() != 0:
            return
        tmp = path + ".tmp"
        torch.save({
            "model": self.model.state_dict(),
            "decoder": self.decoder.state_dict(),
            "optimizer": self.opt.state_dict(),
            "master": self.master,
            "step": self.step_idx,
            "lr_schedule": (self.lr_schedule.to_dict()
                            if self.lr_schedule is not None else None),
            "base_lr": (self.fused_opt.lr if self.fused_opt is not None
                        else self.base_lr),
            "no_decay": self.no_decay,
            "rng": torch.get_rng_state(),
            "cuda_rng": (torch.cuda.get_rng_state()
                         if torch.cuda.is_available() else None),
        }, tmp)
        os.replace(tmp, path)

    def load_checkpoint(self, path: str):
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        # checkpoints from before schedules existed: constant lr, decay on
        if bool(ckpt.get("no_decay", False)) != self.no_decay:
            raise ValueError(
                f"checkpoint was written with no_decay="
                f"{bool(ckpt.get('no_decay', False))}, this trainer has "
                f"no_decay={self.no_decay}")
        self.model.load_state_dict(ckpt["model"])
        self.decoder.load_state_dict(ckpt["decoder"])
        self.opt.load_state_dict(ckpt["optimizer"])
        if "lr_schedule" in ckpt:
            # the step count travels in the optimizer state, so the resumed
            # run continues the schedule where the saved one stopped
            from glom_pytorch_amd.ops.optim import LRSchedule
            d = ckpt["lr_schedule"]
            self.lr_schedule = (LRSchedule.from_dict(d) if d is not None
                                else None)
            self.base_lr = float(ckpt["base_lr"])
            if self.fused_opt is not None:
                self.fused_opt._lr = self.base_lr
                self.fused_opt.schedule = self.lr_schedule
        if ckpt.get("master") is not None and self.master is not None:
            for mw, saved in zip(self.master, ckpt["master"]):
                mw.data.copy_(saved.to(mw.device))
        self.step_idx = ckpt["step"]
        # params follow the restored masters (the fused path reads/writes
        # masters as the source of truth)
        if self.master is not None:
            with torch.no_grad():
                for mw, q in zip(self.master, self._params):
                    q.data.copy_(mw.to(q.dtype))
        torch.set_rng_state(ckpt["rng"])
        if ckpt.get("cuda_rng") is not None and torch.cuda.is_available():
            torch.cuda.set_rng_state(ckpt["cuda_rng"])
        # drop any captured graphs: they bake in old grad/param pointers
        self._graphs.clear()
        return self
