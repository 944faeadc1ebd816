"""Autograd wrappers around the CDNA4 HIP ops + the native Glom forward.

Every hot op of the reference forward is a custom
torch.autograd.Function with hand-written HIP forward AND backward kernels;
autograd only stitches the iteration loop together (and re-traverses it for
losses attached at any (time, level) of the trajectory, as in the
reference's denoising recipe, README.md:56-90).
"""

from __future__ import annotations

import collections
import os

import torch

from glom_pytorch_amd.ops import _load_extension


class PatchEmbedFn(torch.autograd.Function):
    """Patchify + embed GEMM (K1; reference glom_pytorch.py:94-97,114):
    the rearrange runs as a HIP gather kernel into a K-padded (B,N,Kp)
    token matrix and the 588->dim projection on the tuned NT MFMA kernel.
    Backward: split-K TN weight grad, native colsum bias grad, and (only
    when the image itself needs grad) an NN GEMM + scatter back to
    (B,3,H,W)."""

    @staticmethod
    def forward(ctx, img, w, b, patch_size):
        ext = _load_extension()
        tokens, X = ext.patch_embed_fwd(img.contiguous(), w, b, patch_size)
        ctx.save_for_backward(X, w)
        ctx.patch = patch_size
        ctx.img_hw = (img.shape[2], img.shape[3])
        return tokens

    @staticmethod
    def backward(ctx, dTokens):
        ext = _load_extension()
        X, w = ctx.saved_tensors
        need_dimg = ctx.needs_input_grad[0]
        dW, dB, dImg = ext.patch_embed_bwd(
            dTokens.contiguous(), X, w, ctx.patch, ctx.img_hw[0],
            ctx.img_hw[1], need_dimg)
        return (dImg if need_dimg else None), dW, dB, None


class LinearFixedBiasGradFn(torch.autograd.Function):
    """nn.Linear on bf16 GPU tensors with the stock forward and data/weight
    gradients, but the bias gradient from the native two-launch fixed-order
    column sum. Inside overlapped training steps the stock single-launch
    reduction occasionally returned a different block of columns for a
    bitwise identical input (cause not established, see
    docs/ARCHITECTURE.md "Numerics contract"); this one repeats bitwise."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.nn.functional.linear(x, w, b)

    @staticmethod
    def backward(ctx, g):
        ext = _load_extension()
        x, w = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1]).contiguous()
        x2 = x.reshape(-1, x.shape[-1])
        dx = g2.mm(w).view_as(x) if ctx.needs_input_grad[0] else None
        dw = g2.t().mm(x2) if ctx.needs_input_grad[1] else None
        db = ext.colsum(g2) if ctx.needs_input_grad[2] else None
        return dx, dw, db


class ContrastFn(torch.autograd.Function):
    """Column-contrastive loss (``glom_pytorch_amd.contrast``) on (M, D)
    bf16 row matrices, ``M = B * group``. Forward: two reciprocal-norm
    launches, one NT GEMM whose EPI_NCE_FWD epilogue reduces
    ``exp(s - 1/T)`` per (row, column tile) without storing the logits, and
    a fixed-order finish. Backward: per row block, EPI_NCE_BWD recomputes
    the logits and writes ``G'`` (bf16, <= 64 MiB), a split-K NN GEMM forms
    ``G' @ other`` in f32 slices and a row kernel adds them in order,
    applies the normalisation term and the incoming gradient and rounds to
    bf16 once. Saved: the inputs, ``lse`` and both norm vectors."""

    @staticmethod
    def forward(ctx, a, b, group, temperature, all_negatives):
        ext = _load_extension()
        loss, lse, ra, rb = ext.nce_fwd(a, b, group, temperature,
                                        all_negatives)
        ctx.save_for_backward(a, b, lse, ra, rb)
        ctx.cfg = (group, temperature, all_negatives)
        return loss

    @staticmethod
    def backward(ctx, go):
        ext = _load_extension()
        a, b, lse, ra, rb = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        go = go.to(torch.float32).reshape(1).contiguous()
        dA, dB = ext.nce_bwd(go, a, b, lse, ra, rb, *ctx.cfg, need_a,
                             need_b)
        return (dA if need_a else None), (dB if need_b else None), \
            None, None, None


class TrajectoryFn(torch.autograd.Function):
    """return_all trajectory (reference glom_pytorch.py:126,145-148)
    without the torch.stack copy: every step already wrote its output into
    slab[t+1] (and slab[0] holds the initial state), so forward is an
    identity on the slab and backward just slices the incoming gradient
    back to the per-step outputs."""

    @staticmethod
    def forward(ctx, slab, *steps):
        return slab

    @staticmethod
    def backward(ctx, dtraj):
        return (None,) + tuple(dtraj[t] for t in range(dtraj.shape[0]))


class ConeTrajectoryFn(torch.autograd.Function):
    """TrajectoryFn under the loss_level_min promise (backward merge on):
    the loss reads time ``t`` only, so only that step's output is an input
    and every other time gets no gradient at all, instead of an all-zero
    slice that autograd would add to the gradient coming from the next
    step."""

    @staticmethod
    def forward(ctx, slab, step, t):
        ctx.t = t
        return slab

    @staticmethod
    def backward(ctx, dtraj):
        return None, dtraj[ctx.t], None


def trajectory_at(all_levels, t):
    """``all_levels[t]`` of a ``return_all`` forward. Where the forward ran
    with ``loss_level_min`` and the backward merge on, this is the step
    output itself (an alias of the slab's slice that carries the step's
    ``grad_fn``), so the backward of a later ``[:, :, level]`` select fills
    one time slice instead of the whole trajectory. Plain indexing keeps
    working and gives the same values and gradients."""
    steps = getattr(all_levels, "_glom_steps", None)
    if steps is None:
        return all_levels[t]
    return steps[t % len(steps)]


class GroupedFFFn(torch.autograd.Function):
    """Grouped per-level MLP (d -> 4d -> GELU -> d), bottom-up or top-down.

    mode 0 (bottom-up): group 0 consumes `tokens`, group g consumes
    levels[..., g-1, :]  (reference glom_pytorch.py:132-134, without the cat)
    mode 1 (top-down): group g consumes levels[..., g+1, :] + pos; the pos
    add is materialized once per call by k_add_pos (glom_pytorch.py:136).
    """

    @staticmethod
    def forward(ctx, tokens, levels, pos, w1, b1, w2, b2, mode):
        ext = _load_extension()
        Y, Hpre, Hact, td_in = ext.grouped_ff_fwd(tokens, levels, pos, w1,
                                                  b1, w2, b2, mode)
        ctx.save_for_backward(tokens, levels, pos, w1, w2, Hpre, Hact,
                              td_in)
        ctx.mode = mode
        return Y

    @staticmethod
    def backward(ctx, dY):
        ext = _load_extension()
        tokens, levels, pos, w1, w2, Hpre, Hact, td_in = ctx.saved_tensors
        dTokens, dLevels, dW1, dB1, dW2, dB2 = ext.grouped_ff_bwd(
            dY.contiguous(), tokens, levels, pos, w1, w2, Hpre, Hact,
            ctx.mode, None, None, td_in)
        dPos = None
        if ctx.mode == 1 and pos is not None and ctx.needs_input_grad[2]:
            # pos was added to every top-down group input; its grad is the
            # sum of the level-slice grads over batch and groups (native
            # deterministic reduction).
            dPos = ext.dpos(dLevels)
        if ctx.mode == 0:
            return dTokens, dLevels, None, dW1, dB1, dW2, dB2, None
        return None, dLevels, dPos, dW1, dB1, dW2, dB2, None


class ConsensusFn(torch.autograd.Function):
    """Consensus attention across patch columns (glom_pytorch.py:38-73)."""

    @staticmethod
    def forward(ctx, levels, attend_self, mask):
        ext = _load_extension()
        out, probs, rnorm = ext.consensus_fwd(levels, attend_self, mask)
        ctx.save_for_backward(levels, probs, rnorm, mask)
        ctx.attend_self = attend_self
        return out

    @staticmethod
    def backward(ctx, dOut):
        ext = _load_extension()
        levels, probs, rnorm, mask = ctx.saved_tensors
        dLevels = ext.consensus_bwd(dOut.contiguous(), levels, probs, rnorm,
                                    ctx.attend_self, mask)
        return dLevels, None, None


class LevelMixFn(torch.autograd.Function):
    """(prev + bu + pad(td) + cons) / [4,..,4,3]  (glom_pytorch.py:141-144)."""

    @staticmethod
    def forward(ctx, levels, bu, td, cons):
        ext = _load_extension()
        return ext.level_mix_fwd(levels, bu, td, cons)

    @staticmethod
    def backward(ctx, dout):
        ext = _load_extension()
        dmix, dtd = ext.level_mix_bwd(dout.contiguous())
        # prev/bu/cons share the same scaled gradient; hand the engine
        # distinct view objects so it can never steal/accumulate into one
        # buffer in place on behalf of another input.
        return dmix, dmix.view_as(dmix), dtd, dmix.view_as(dmix)


class GlomStepFn(torch.autograd.Function):
    """One full GLOM iteration (reference glom_pytorch.py:131-145) as a
    single autograd node: forward chains bottom-up / top-down / consensus /
    level-mix in one extension call; backward sums the four levels-gradient
    contributions in one fused kernel instead of three engine
    accumulations."""

    _streams = None

    @staticmethod
    def _side_streams():
        if GlomStepFn._streams is None:
            GlomStepFn._streams = (torch.cuda.Stream(), torch.cuda.Stream(),
                                   torch.cuda.Stream())
        return GlomStepFn._streams

    @staticmethod
    def forward(ctx, tokens, levels, pos, bw1, bb1, bw2, bb2,
                tw1, tb1, tw2, tb2, attend_self, mask,
                bw1t, bw2t, tw1t, tw2t, slab_ref=None,
                save_for_bwd=True, cone=None, carry=None):
        # slab_ref: optional (slab, idx) — write the step output straight
        # into the preallocated trajectory slab (untracked alias return)
        # save_for_bwd: False on forward-only steps (decided by glom_step,
        # outside this Function) — the FF pre-activations, which only the
        # backward reads, are then neither allocated nor written
        # cone: None, or (lo, t) — glom_forward's promise that the gradient
        # arriving at this step (iteration t) is zero in levels < lo. The
        # backward then runs the groups / levels >= lo only. With lo = L-1
        # no top-down group is live, so its pre-activations are not kept
        # carry: None, or glom_forward's _LoopCarry (not differentiable):
        # the kept token-MLP output, what the previous step's mix prepared
        # for this one, and what this step's mix is to prepare
        ext = _load_extension()
        bu0 = carry.bu0 if carry is not None and carry.skip0 else None
        td_ready = carry.td_in if carry is not None else None
        rn_ready = carry.rnorm if carry is not None else None
        emit = carry is not None and carry.emit
        slab, sidx = slab_ref if slab_ref is not None else (None, 0)
        lo = cone[0] if cone is not None else 0
        save_td = save_for_bwd and (lo < levels.size(2) - 1
                                    or FORCE_SAVE_FOR_BWD)
        # the three per-iteration chains (bottom-up MLP, top-down MLP,
        # consensus attention) only depend on `levels`; forking them onto
        # side streams overlaps their tail waves (+10% forward throughput
        # measured on inference).
        cur = torch.cuda.current_stream()
        s_td, s_at, _ = GlomStepFn._side_streams()
        ev = torch.cuda.Event()
        ev.record(cur)
        buY, bhp, bha, _ = ext.grouped_ff_fwd(tokens, levels, None, bw1, bb1,
                                              bw2, bb2, 0, save_for_bwd,
                                              bu0 is not None)
        with torch.cuda.stream(s_td):
            s_td.wait_event(ev)
            tdY, thp, tha, tdin = ext.grouped_ff_fwd(None, levels, pos, tw1,
                                                     tb1, tw2, tb2, 1,
                                                     save_td, False,
                                                     td_ready)
        with torch.cuda.stream(s_at):
            s_at.wait_event(ev)
            cons, probs, rnorm = ext.consensus_fwd(levels, attend_self,
                                                   mask, rn_ready)
        cur.wait_stream(s_td)
        cur.wait_stream(s_at)
        # boundary tensors crossing back to the main stream: pin their
        # blocks until the main stream catches up (allocator safety)
        for t in (tdY, thp, tha, tdin, cons, probs, rnorm):
            if t.numel():
                t.record_stream(cur)
        if emit:
            out, td_next, rn_next = ext.level_mix_fwd_next(
                levels, buY, tdY, cons, slab, sidx, bu0, pos)
            carry.set_next(td_next, rn_next)
        else:
            out = ext.level_mix_fwd(levels, buY, tdY, cons, slab, sidx, bu0)
            if carry is not None:
                carry.set_next(None, None)
        if carry is not None and carry.hoist and carry.bu0 is None:
            # this step ran every group: keep its token-MLP output (a view
            # into Y, row stride L*d) for the rest of the forward
            carry.bu0 = buY[:, :, 0, :]
        ctx.save_for_backward(tokens, levels, pos, bw1, bw2, tw1, tw2,
                              bhp, bha, thp, tha, probs, rnorm, mask,
                              bw1t, bw2t, tw1t, tw2t, tdin)
        ctx.attend_self = attend_self
        ctx.cone = cone
        ctx.bwd = carry.bwd if carry is not None and cone is not None \
            else None
        return out

    @staticmethod
    def _backward_merged(ctx, dnew):
        """The 3-way fork under a level cone with the backward merge on
        (docs/ARCHITECTURE.md "Backward merge"): dmix comes from the next
        step's merge kernel when autograd hands that step's dLevels through
        untouched; the top-down chain reads dmix with row stride L*d; dB2 is
        summed once; no chain zero-fills what it does not write, because
        grad_merge knows each contribution's range."""
        ext, sv, lo = _bwd_begin(ctx, dnew)
        levels, t = sv.levels, ctx.cone[1]
        L, d = levels.size(2), levels.size(3)
        td_live = lo < L - 1
        cur = torch.cuda.current_stream()
        s_td, s_at, _ = GlomStepFn._side_streams()
        dmix = ctx.bwd.take(dnew, lo)
        if dmix is None:
            dmix = ext.level_mix_bwd(dnew.contiguous(), lo, False)[0]
        ev = torch.cuda.Event()
        ev.record(cur)
        # the attention chain is the shortest of the three: it also carries
        # the one dB2 column sum that both FF nets share
        with torch.cuda.stream(s_at):
            s_at.wait_event(ev)
            dAttn = ext.consensus_bwd(dmix, levels, sv.probs, sv.rnorm,
                                      ctx.attend_self, sv.mask, lo, True)
            db2_bu, db2_td = ext.db2_cone(dmix, lo)
        dmix.record_stream(s_at)
        bu = ext.grouped_ff_bwd(dmix, sv.tokens, levels, None, sv.bw1,
                                sv.bw2, sv.bhp, sv.bha, 0, sv.bw1t, sv.bw2t,
                                None, lo, 0, db2_bu, True)
        # no live top-down group (lo + 1 == L): zero fills, no side stream
        with torch.cuda.stream(s_td if td_live else None):
            if td_live:
                s_td.wait_event(ev)
            td = ext.grouped_ff_bwd(dmix, None, levels, sv.pos, sv.tw1,
                                    sv.tw2, sv.thp, sv.tha, 1, sv.tw1t,
                                    sv.tw2t, sv.tdin, lo, L * d, db2_td, True)
            dPos = ext.dpos(td[1], lo + 1)
        if td_live:
            dmix.record_stream(s_td)
            cur.wait_stream(s_td)
        cur.wait_stream(s_at)
        back = [dAttn, db2_bu, db2_td]
        if td_live:
            back += list(td) + [dPos]
        for x in back:
            if x is not None and x.numel():
                x.record_stream(cur)
        want_next = t > 0
        dLevels, dmix_next = ext.grad_merge(dmix, bu[1], td[1], dAttn, lo,
                                            ctx.bwd.posz, want_next)
        if want_next:
            ctx.bwd.put(dLevels, dmix_next, max(lo - 1, 0))
        return _step_grads(bu[0], dLevels, dPos, bu[2], bu[3], bu[4], bu[5],
                           td[2], td[3], td[4], td[5])

    @staticmethod
    def backward(ctx, dnew):
        # the environment is read again here, a prepared carry is not enough
        path = _bwd_path(merge=ctx.bwd is not None)
        return getattr(GlomStepFn, "_backward_" + path)(ctx, dnew)

    @staticmethod
    def _backward_single(ctx, dnew):
        """One extension call on the current stream."""
        ext, sv, lo = _bwd_begin(ctx, dnew)
        # the saved tensors in their order, attend_self before the mask
        return _step_grads(*ext.glom_step_bwd(
            dnew.contiguous(), *sv[:13], ctx.attend_self, *sv[13:], lo))

    @staticmethod
    def _backward_fork3(ctx, dnew):
        """Bottom-up chain on the current stream, top-down and attention
        chains on side streams. Groups / levels below lo carry an exactly-
        zero gradient; the ops skip them and fill in the zeros. The top-down
        MLP has groups 0..L-2: with lo = L-1 none is live (td_live)."""
        ext, sv, lo = _bwd_begin(ctx, dnew)
        levels, L = sv.levels, sv.levels.size(2)
        td_lo, td_live = min(lo, L - 1), lo < L - 1
        cur = torch.cuda.current_stream()
        s_td, s_at, _ = GlomStepFn._side_streams()
        dmix, dtd = ext.level_mix_bwd(dnew.contiguous())
        ev = torch.cuda.Event()
        ev.record(cur)
        bu = ext.grouped_ff_bwd(dmix, sv.tokens, levels, None, sv.bw1,
                                sv.bw2, sv.bhp, sv.bha, 0, sv.bw1t, sv.bw2t,
                                None, lo)
        # no live top-down group: only zero fills, no side stream
        with torch.cuda.stream(s_td if td_live else None):
            if td_live:
                s_td.wait_event(ev)
            td = ext.grouped_ff_bwd(dtd, None, levels, sv.pos, sv.tw1,
                                    sv.tw2, sv.thp, sv.tha, 1, sv.tw1t,
                                    sv.tw2t, sv.tdin, td_lo)
        if td_live:
            dtd.record_stream(s_td)
        with torch.cuda.stream(s_at):
            s_at.wait_event(ev)
            dAttn = ext.consensus_bwd(dmix, levels, sv.probs, sv.rnorm,
                                      ctx.attend_self, sv.mask, lo)
        dmix.record_stream(s_at)
        if td_live:
            cur.wait_stream(s_td)
        cur.wait_stream(s_at)
        for t in (list(td) if td_live else []) + [dAttn]:
            if t is not None and t.numel():
                t.record_stream(cur)
        dLevels = torch.empty_like(levels)
        ext.add4_into(dmix, bu[1], td[1], dAttn, dLevels)
        dPos = ext.dpos(td[1])
        return _step_grads(bu[0], dLevels, dPos, bu[2], bu[3], bu[4], bu[5],
                           td[2], td[3], td[4], td[5])

    @staticmethod
    def _backward_fork4(ctx, dnew):
        """fork3 with the weight gradients on a fourth stream: measured
        slightly SLOWER (sync overhead), kept for future tuning."""
        ext, sv, lo = _bwd_begin(ctx, dnew)
        levels, pos = sv.levels, sv.pos
        B, N, L = levels.size(0), levels.size(1), levels.size(2)
        td_lo, td_live = min(lo, L - 1), lo < L - 1
        cur = torch.cuda.current_stream()
        s_td, s_at, s_w = GlomStepFn._side_streams()
        dmix, dtd = ext.level_mix_bwd(dnew.contiguous())
        ev0 = torch.cuda.Event()
        ev0.record(cur)
        bu_dh, bu_db1 = ext.ff_bwd_dh(dmix, sv.bw2t, sv.bhp, lo)
        ev_bu = torch.cuda.Event()
        ev_bu.record(cur)
        if td_live:
            with torch.cuda.stream(s_td):
                s_td.wait_event(ev0)
                td_dh, td_db1 = ext.ff_bwd_dh(dtd, sv.tw2t, sv.thp, td_lo)
                ev_td = torch.cuda.Event()
                ev_td.record(s_td)
        else:
            # no live top-down group: the op only zero-fills its six
            # results; neither s_td nor the top-down half of s_w is used
            (_, td_dl, td_w1, td_db1, td_w2, td_b2) = ext.grouped_ff_bwd(
                dtd, None, levels, pos, sv.tw1, sv.tw2, sv.thp, sv.tha, 1,
                sv.tw1t, sv.tw2t, sv.tdin, td_lo)
        with torch.cuda.stream(s_at):
            s_at.wait_event(ev0)
            dAttn = ext.consensus_bwd(dmix, levels, sv.probs, sv.rnorm,
                                      ctx.attend_self, sv.mask, lo)
        with torch.cuda.stream(s_w):
            s_w.wait_event(ev_bu)
            bu_w1, bu_w2, bu_b2 = ext.ff_bwd_dw(dmix, bu_dh, sv.tokens,
                                                levels, None, sv.bha, 0,
                                                None, lo)
            if td_live:
                s_w.wait_event(ev_td)
                td_w1, td_w2, td_b2 = ext.ff_bwd_dw(dtd, td_dh, None,
                                                    levels, pos, sv.tha, 1,
                                                    sv.tdin, td_lo)
        bu_dt, bu_dl = ext.ff_bwd_dx(bu_dh, sv.bw1t, sv.tokens, B, N, L, 0,
                                     lo)
        if td_live:
            with torch.cuda.stream(s_td):
                _, td_dl = ext.ff_bwd_dx(td_dh, sv.tw1t, None, B, N, L, 1,
                                         td_lo)
        # cross-stream block pinning
        pins = [(dmix, s_at), (dmix, s_w), (bu_dh, s_w)]
        if td_live:
            pins += [(dtd, s_td), (dtd, s_w), (td_dh, s_w)]
        for t, st in pins:
            t.record_stream(st)
        if td_live:
            cur.wait_stream(s_td)
        cur.wait_stream(s_at)
        cur.wait_stream(s_w)
        back = [dAttn, bu_w1, bu_w2, bu_b2]
        if td_live:
            back += [td_db1, td_dl, td_w1, td_w2, td_b2]
        for t in back:
            t.record_stream(cur)
        dLevels = torch.empty_like(levels)
        ext.add4_into(dmix, bu_dl, td_dl, dAttn, dLevels)
        dPos = ext.dpos(td_dl)
        return _step_grads(bu_dt, dLevels, dPos, bu_w1, bu_db1, bu_w2, bu_b2,
                           td_w1, td_db1, td_w2, td_b2)


# GlomStepFn's saved tensors, in save_for_backward order
_Saved = collections.namedtuple(
    "_Saved", "tokens levels pos bw1 bw2 tw1 tw2 bhp bha thp tha probs rnorm "
              "mask bw1t bw2t tw1t tw2t tdin")


def _step_grads(*grads):
    """Eleven real gradients, then None for GlomStepFn's ten other inputs."""
    return grads + (None,) * 10


def _bwd_path(merge=False):
    """'single' (GLOM_NO_BWD_STREAMS=1, which wins), 'fork4' (GLOM_BWD_FORK
    set to anything but 3), else 'fork3', or 'merged' where asked for."""
    if os.environ.get("GLOM_NO_BWD_STREAMS", "0") == "1":
        return "single"
    if os.environ.get("GLOM_BWD_FORK", "3") != "3":
        return "fork4"
    return "merged" if merge else "fork3"


def _bwd_begin(ctx, dnew):
    """(ext, saved tensors, first live level), after the check mode's test."""
    lo = ctx.cone[0] if ctx.cone is not None else 0
    if lo > 0 and CHECK_LEVEL_CONE:
        _check_cone(dnew, lo, ctx.cone[1])
    return _load_extension(), _Saved(*ctx.saved_tensors), lo


def _transposed_weights(model):
    """Per-group W^T copies for the backward NT GEMMs, computed ONCE per
    forward (they are loop constants across the T iterations)."""
    with torch.no_grad():
        L, d = model.levels, model.dim
        bw1 = model.bottom_up.net[1].weight[..., 0]
        bw2 = model.bottom_up.net[3].weight[..., 0]
        tw1 = model.top_down.net[1].weight[..., 0]
        tw2 = model.top_down.net[3].weight[..., 0]
        m4 = bw1.shape[0] // L
        return (
            bw1.view(L, m4, d).transpose(1, 2).contiguous(),
            bw2.view(L, d, m4).transpose(1, 2).contiguous(),
            tw1.view(L - 1, m4, d).transpose(1, 2).contiguous(),
            tw2.view(L - 1, d, m4).transpose(1, 2).contiguous(),
        )


# Test / A-B hook: True keeps the FF pre-activations on every step, as
# before forward-only steps learned to skip them (GLOM_SAVE_HPRE=1).
FORCE_SAVE_FOR_BWD = os.environ.get("GLOM_SAVE_HPRE", "0") == "1"


# Level-cone check mode (set_check_level_cone / GLOM_CHECK_LEVEL_CONE=1):
# before each step's backward, test with one host sync that the incoming
# gradient really is zero below the promised level. Off by default.
CHECK_LEVEL_CONE = os.environ.get("GLOM_CHECK_LEVEL_CONE", "0") == "1"


def set_check_level_cone(on: bool) -> None:
    global CHECK_LEVEL_CONE
    CHECK_LEVEL_CONE = bool(on)


# Loop invariants (docs/ARCHITECTURE.md "Loop invariants"), each with a
# switch that is read once per glom_forward call, so both settings can be
# compared within one process:
#   token hoist  set_token_hoist / GLOM_NO_TOKEN_HOIST=1 — bottom-up group 0
#                (the token MLP) runs in iteration 0 and again only at steps
#                whose backward reads its pre-activations
#   mix fusion   set_mix_fusion / GLOM_NO_MIX_FUSION=1 — the level mix also
#                writes the next iteration's td_in and rnorm
TOKEN_HOIST = True
MIX_FUSION = True


def set_token_hoist(on: bool) -> None:
    global TOKEN_HOIST
    TOKEN_HOIST = bool(on)


def set_mix_fusion(on: bool) -> None:
    global MIX_FUSION
    MIX_FUSION = bool(on)


# Backward merge (docs/ARCHITECTURE.md "Backward merge"): set_bwd_merge /
# GLOM_NO_BWD_MERGE=1, read once per glom_forward like the two above. Off
# restores every launch of the unmerged backward, the dense trajectory
# gradient included.
BWD_MERGE = True


def set_bwd_merge(on: bool) -> None:
    global BWD_MERGE
    BWD_MERGE = bool(on)


class _BwdCarry:
    """The backward's mirror of _LoopCarry: what step t's backward leaves
    for step t-1's. ``put`` keeps (dLevels_t, dmix_next, first level of
    dmix_next that was written); ``take`` hands dmix_next out only if the
    gradient autograd delivers IS dLevels_t (same storage, shape and
    strides, so nothing was added to it and no hook replaced it) and the
    taker's cone starts no lower than what was written. The pair is dropped
    after one ``take`` either way; the caller then computes dmix from the
    gradient it was given. No host synchronisation: pointer compares only.

    posz: the forward returns the trajectory, so the unmerged path would
    add an all-zero slice to every step's dLevels (-0 becomes +0)."""

    def __init__(self, posz):
        self.posz = bool(posz)
        self._pair = None

    def put(self, dlevels, dmix_next, written_from):
        self._pair = (dlevels, dmix_next, written_from)

    def take(self, dnew, lo):
        pair, self._pair = self._pair, None
        if pair is None:
            return None
        dl, dm, written_from = pair
        same = (dnew.data_ptr() == dl.data_ptr() and dnew.dtype == dl.dtype
                and dnew.shape == dl.shape and dnew.stride() == dl.stride())
        return dm if same and lo >= written_from else None


class _LoopCarry:
    """What one glom_forward call carries from iteration to iteration
    besides `levels`. None of it is differentiable.

    bu0:    (B,N,d) view of iteration 0's bottom-up output, level 0; set by
            the first step that runs every group, then read by the level
            mix of every step that skips group 0
    skip0:  decided per step by glom_step (outside Function.forward)
    td_in, rnorm: written by the previous step's mix for this step, or None
    emit:   this step's mix is to write them for the next step"""

    def __init__(self, levels):
        two = levels.size(2) >= 2
        self.hoist = (two and TOKEN_HOIST and
                      os.environ.get("GLOM_NO_TOKEN_HOIST", "0") != "1")
        self.fuse = (two and MIX_FUSION and
                     os.environ.get("GLOM_NO_MIX_FUSION", "0") != "1")
        self.bu0 = None
        self.skip0 = False
        self.td_in = None
        self.rnorm = None
        self.emit = False
        self.bwd = None     # _BwdCarry, set by glom_forward when merging

    def set_next(self, td_in, rnorm):
        # the mix returns empty tensors where it does not emit (d != 512)
        ok = td_in is not None and td_in.numel() > 0
        self.td_in = td_in if ok else None
        self.rnorm = rnorm if ok else None

    def tensors(self):
        return [t for t in (self.bu0, self.td_in, self.rnorm)
                if t is not None]


def level_cone_lo(loss_level_min: int, grad_iters: int, t: int) -> int:
    """Lowest level in which the gradient arriving at iteration t (that is,
    at trajectory time t + 1) can be non-zero, when the loss reads time
    grad_iters at levels >= loss_level_min only: every iteration further
    back widens the range by one level (bottom-up group g feeds level g
    from level g - 1; top-down, consensus and the residual never reach
    further down)."""
    return max(0, loss_level_min - (grad_iters - 1 - t))


def _check_cone(dnew, lo, t):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(
            "the level-cone check synchronises with the host and cannot "
            "run under stream capture; turn it off (set_check_level_cone"
            "(False), GLOM_CHECK_LEVEL_CONE=0) or run the step uncaptured")
    bad = dnew[:, :, :lo].ne(0).any(dim=3).any(dim=1).any(dim=0).tolist()
    if any(bad):
        lvl = bad.index(True)
        raise RuntimeError(
            f"loss_level_min promise broken: the gradient arriving at "
            f"iteration {t} is non-zero in level {lvl}, below the first "
            f"level ({lo}) that loss_level_min allows there")


def _needs_bwd(*tensors):
    """Will autograd record a backward through a step on these inputs?
    Must be asked OUTSIDE Function.forward (grad mode is off in there)."""
    if FORCE_SAVE_FOR_BWD:
        return True
    return torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in tensors)


def _step_args(model, tokens, levels, pos):
    """The first eleven arguments of GlomStepFn and ext.glom_step_fwd."""
    bw = model.bottom_up.net
    tw = model.top_down.net
    return (tokens, levels, pos,
            bw[1].weight[..., 0], bw[1].bias, bw[3].weight[..., 0],
            bw[3].bias,
            tw[1].weight[..., 0], tw[1].bias, tw[3].weight[..., 0],
            tw[3].bias)


def glom_step(model, tokens, levels, pos, mask, wts=None, slab_ref=None,
              cone=None, carry=None):
    wts = wts or (None,) * 4
    args = _step_args(model, tokens, levels, pos)
    if carry is not None:
        # group 0 may be skipped when nothing will read this step's group-0
        # Hpre / Hact: no backward is recorded, or its cone starts above 0
        records_bwd = torch.is_grad_enabled() and any(
            t is not None and t.requires_grad for t in args)
        carry.skip0 = carry.bu0 is not None and (
            not records_bwd or (cone is not None and cone[0] >= 1))
    return GlomStepFn.apply(
        *args, model.attention.attend_self, mask, *wts, slab_ref,
        _needs_bwd(*args), cone, carry)


_TAIL_STREAM = None
# what the tail reads besides the slab: held from glom_forward until
# join_tail_stream (the kept token-MLP output, the last mix's extras)
_TAIL_KEEP = []


def _tail_stream():
    global _TAIL_STREAM
    if _TAIL_STREAM is None:
        _TAIL_STREAM = torch.cuda.Stream()
    return _TAIL_STREAM


def join_tail_stream():
    """Block the current stream on the overlap-tail stream. Callers that
    requested ``overlap_tail`` MUST call this before reading the
    trajectory's post-grad_iters slices or mutating model weights (the
    trainer joins right before the optimizer update)."""
    if _TAIL_STREAM is not None:
        torch.cuda.current_stream().wait_stream(_TAIL_STREAM)
    del _TAIL_KEEP[:]


def glom_forward(model, img, iters, levels=None, return_all=False,
                 grad_iters=None, overlap_tail=False, loss_level_min=None):
    """grad_iters (optional): iterations >= grad_iters run under no_grad.
    Forward VALUES are identical; gradients stop flowing through those
    steps. When a loss only touches trajectory times <= grad_iters (the
    reference's denoising recipe decodes at t=7 of 12), the skipped
    backward contributions are exactly zero — autograd would otherwise
    backprop zeros through every post-loss iteration (reference
    glom_pytorch.py:131-148 has the same dead work).

    loss_level_min (optional, needs grad_iters): the caller promises that
    the loss reads the trajectory ONLY at time grad_iters and ONLY at
    levels >= loss_level_min. One iteration moves information by one level
    at most, so the gradient arriving at iteration t is exactly zero in
    levels below lo_t = max(0, loss_level_min - (grad_iters - 1 - t)); the
    backward skips those groups and levels and fills in their zeros. Same
    values and gradients; a broken promise silently drops gradient unless
    the check mode (set_check_level_cone) is on."""
    from glom_pytorch_amd.utils.profiling import trace_range
    if loss_level_min is not None:
        if grad_iters is None:
            raise ValueError("loss_level_min requires grad_iters")
        if not 0 <= loss_level_min < model.levels:
            raise ValueError("loss_level_min must be a level index")
    b = img.shape[0]
    with trace_range("glom/patch_embed"):
        # K1: hand-written patchify + NT MFMA GEMM, once per forward
        emb = model.image_to_tokens[1]
        tokens = PatchEmbedFn.apply(img, emb.weight, emb.bias,
                                    model.patch_size)
    n = tokens.shape[1]
    pos = model.pos_emb.weight
    mask = (model.attention.non_local_mask
            if model.attention.local_consensus_radius > 0 else None)

    if levels is None:
        levels = model.init_levels.view(1, 1, model.levels, model.dim) \
            .expand(b, n, model.levels, model.dim).contiguous()
    else:
        levels = levels.contiguous()

    wts = _transposed_weights(model) if torch.is_grad_enabled() else None

    # return_all: steps write straight into a preallocated (T+1) slab —
    # no torch.stack copy at the end (SURVEY.md §2.3 note)
    slab = None
    if return_all:
        slab = torch.empty((iters + 1,) + tuple(levels.shape),
                           device=levels.device, dtype=levels.dtype)
        with torch.no_grad():
            slab[0].copy_(levels)

    # opt-in: run the forward-only tail (iterations >= grad_iters)
    # CONCURRENTLY with the caller's backward on a dedicated stream. The
    # tail never feeds the loss, and the caller joins (join_tail_stream)
    # before the optimizer mutates weights, so this is race-free.
    overlap = (overlap_tail and grad_iters is not None
               and grad_iters < iters and img.is_cuda
               and torch.is_grad_enabled())
    n_sync = grad_iters if overlap else iters

    carry = _LoopCarry(levels)
    # backward merge: needs the promise, 16-byte level rows, a top-down net
    # and the default 3-way backward fork
    merge = (loss_level_min is not None and BWD_MERGE
             and os.environ.get("GLOM_NO_BWD_MERGE", "0") != "1"
             and _bwd_path(merge=True) == "merged"
             and model.dim % 8 == 0 and model.levels >= 2
             and 0 < grad_iters <= iters and torch.is_grad_enabled())
    if merge:
        carry.bwd = _BwdCarry(posz=return_all)

    steps = [levels]
    with trace_range(f"glom/iterate x{iters}"):
        for t in range(n_sync):
            sref = (slab, t + 1) if slab is not None else None
            # the last iteration's mix has no successor to prepare for
            carry.emit = carry.fuse and t < iters - 1
            with trace_range(f"glom/step{t}"):
                if grad_iters is not None and t >= grad_iters:
                    with torch.no_grad():
                        levels = glom_step(model, tokens, levels, pos,
                                           mask, wts, sref, None, carry)
                else:
                    cone = None
                    if loss_level_min is not None:
                        cone = (level_cone_lo(loss_level_min, grad_iters,
                                              t), t)
                    levels = glom_step(model, tokens, levels, pos, mask,
                                       wts, sref, cone, carry)
            if return_all:
                steps.append(levels)
        if overlap:
            ext = _load_extension()
            s_tail = _tail_stream()
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            # the carried tensors were written on the current stream and are
            # read on s_tail: pin their blocks there, and hold them until
            # join_tail_stream
            for kept in carry.tensors():
                kept.record_stream(s_tail)
            _TAIL_KEEP[:] = carry.tensors()
            with torch.no_grad(), torch.cuda.stream(s_tail):
                s_tail.wait_event(ev)
                for t in range(n_sync, iters):
                    emit = carry.fuse and t < iters - 1
                    outs = ext.glom_step_fwd(
                        *_step_args(model, tokens, levels, pos),
                        model.attention.attend_self, mask, slab, t + 1,
                        FORCE_SAVE_FOR_BWD, carry.bu0, carry.td_in,
                        carry.rnorm, emit)
                    levels = outs[0]
                    if emit:
                        carry.set_next(outs[8], outs[9])
                    else:
                        carry.set_next(None, None)
                    if return_all:
                        steps.append(levels)
                if slab is not None:
                    slab.record_stream(s_tail)

    if return_all:
        if merge:
            traj = ConeTrajectoryFn.apply(slab, steps[grad_iters],
                                          grad_iters)
            traj._glom_steps = steps
            return traj
        return TrajectoryFn.apply(slab, *steps)
    return levels
