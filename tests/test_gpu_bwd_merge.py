"""Backward merge: one cone-aware kernel for the level chain of the backward.

Everything here is bitwise: tensors are compared on their int16 view, so the
sign of a zero counts. The op-level tests compare each new kernel or op
option with the composition of launches it replaces; the model-level tests
compare the switch on with the switch off in one process.

Shapes. ``grad_merge``: (1,9,2,8) (one top-down group, 144 elements, less
than a block), (2,9,3,8), (2,16,6,512) (384 blocks). Strided ``dY``: the
generic kernels at M=18 d=8 m4=32 L=3, and B=32 N=256 L=6 d=512 m4=2048, the
shape at which ``tests/test_gpu_level_cone.py`` pins the dispatch: dH runs on
nt5p (8*16*5 = 640 blocks), the top-down dX on nt8p (2*32*5 = 320 >= 256)
and dW1 / dW2 (K = 8192, 320 and 320 tiles) on split-K ``gemm_tn_tr``; no
smaller M reaches the nt8p gate with L = 6, d = 512.
"""

import functools

import pytest
import torch

from glom_pytorch_amd import Glom

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"
BF = torch.bfloat16
OUT6 = ("dTokens", "dLevels", "dW1", "dB1", "dW2", "dB2")
NAN_BITS = 0x7FC1        # a quiet NaN with a payload bit
NEG_ZERO = -32768        # 0x8000 as int16


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ranges(lo, L):
    """Level ranges of (dmix, bottom-up, top-down, dAttn) and the first
    level that is not dead, for a step whose first live level is lo."""
    return ((lo, L), (max(lo, 1) - 1, L - 1), (lo + 1, L), (lo, L)), \
        max(lo - 1, 0)


# ------------------------- 1. grad_merge ------------------------------- #

@functools.lru_cache(maxsize=None)
def _merge_inputs(B, N, L, d):
    """Four random contributions with planted zeros: +0 in one, -0 in one,
    and positions where all four are -0 (the only way to a -0 sum)."""
    g = torch.Generator(device=DEV).manual_seed(11 + L + d)
    xs = [torch.randn(B, N, L, d, device=DEV, generator=g).to(BF)
          for _ in range(4)]
    flat = [x.view(-1) for x in xs]
    n = flat[0].numel()
    pick = torch.randperm(n, device=DEV, generator=g)
    k = max(n // 16, 4)
    for i, f in enumerate(flat):
        f[pick[i * k:(i + 1) * k]] = 0.0                 # +0 in one operand
        f[pick[(4 + i) * k:(5 + i) * k]] = -0.0          # -0 in one operand
    for f in flat:
        f[pick[8 * k:9 * k]] = -0.0                      # all four -0
        f[pick[9 * k:10 * k]] = 0.0                      # all four +0
    # mixed: -0, -0, +0, -0 must give +0
    for i, f in enumerate(flat):
        f[pick[10 * k:11 * k]] = 0.0 if i == 2 else -0.0
    assert (_bits(xs[0]) == NEG_ZERO).any()
    return tuple(xs)


def _composition(xs, lo, L, posz, want_next):
    """What grad_merge replaces: the unmerged ops zero-fill (+0) what they
    do not write, add4 sums everything, autograd adds the all-zero
    trajectory slice (where a trajectory exists) and the next backward
    starts with level_mix_bwd."""
    ext = _ext()
    ranges, _ = _ranges(lo, L)
    filled = []
    for x, (r0, r1) in zip(xs, ranges):
        y = torch.zeros_like(x)
        y[:, :, r0:r1] = x[:, :, r0:r1]
        filled.append(y)
    out = torch.empty_like(xs[0])
    ext.add4_into(*filled, out)
    if posz:
        out = out + torch.zeros_like(out)
    nxt = ext.level_mix_bwd(out)[0] if want_next else None
    return out, nxt


@pytest.mark.parametrize("posz", [False, True], ids=["no_traj", "traj"])
@pytest.mark.parametrize("want_next", [False, True], ids=["plain", "next"])
@pytest.mark.parametrize("shape", [(1, 9, 2, 8), (2, 9, 3, 8),
                                   (2, 16, 6, 512)], ids=str)
def test_grad_merge_equals_add4_zero_add_mix_bwd(shape, want_next, posz):
    ext = _ext()
    B, N, L, d = shape
    xs = _merge_inputs(*shape)
    seen_neg_zero = False
    for lo in range(L + 1):
        ranges, first = _ranges(lo, L)
        # out-of-range slices hold NaNs: a load of one would show
        poisoned = []
        for x, (r0, r1) in zip(xs, ranges):
            y = torch.full_like(x.view(torch.int16), NAN_BITS).view(BF)
            y[:, :, r0:r1] = x[:, :, r0:r1]
            poisoned.append(y)
        # outputs land in poisoned memory too: blocks just freed are what
        # the allocator hands out next
        junk = [torch.full_like(xs[0].view(torch.int16), NAN_BITS)
                for _ in range(2)]
        del junk
        got, got_next = ext.grad_merge(*poisoned, lo, posz, want_next)
        ref, ref_next = _composition(xs, lo, L, posz, want_next)
        torch.cuda.synchronize()
        assert _same(got, ref), (shape, lo)
        assert (_bits(got[:, :, :first]) == 0).all(), (shape, lo)
        seen_neg_zero |= bool((_bits(got) == NEG_ZERO).any())
        if want_next:
            assert got_next.shape == got.shape
            assert _same(got_next[:, :, first:], ref_next[:, :, first:]), \
                (shape, lo)
        else:
            assert got_next.numel() == 0
    # the planted all -0 positions survive exactly where no zero is added
    # (all four contributions are in range at levels 1..L-2 of lo = 0)
    if posz:
        assert not seen_neg_zero
    elif L >= 3:
        assert seen_neg_zero


def test_mix_bwd_lo_writes_the_live_levels_only():
    ext = _ext()
    g = torch.Generator(device=DEV).manual_seed(3)
    for B, N, L, d in [(1, 9, 2, 8), (2, 16, 6, 512)]:
        dout = torch.randn(B, N, L, d, device=DEV, generator=g).to(BF)
        ref, ref_td = ext.level_mix_bwd(dout)
        assert _same(ref_td, ref[:, :, :L - 1])     # dtd is a copy of dmix
        for lo in range(L + 1):
            got, none = ext.level_mix_bwd(dout, lo, False)
            assert none.numel() == 0
            assert _same(got[:, :, lo:], ref[:, :, lo:]), (L, d, lo)


# ------------------ 2. strided dY, dB2, no-fill, dpos ------------------ #

@functools.lru_cache(maxsize=None)
def _ff_case(B, N, L, d, mode):
    """One grouped FF call: inputs and the forward's saved tensors. The
    incoming gradient is a dmix-shaped (B,N,L,d) tensor shared by both
    modes; mode 1's compact dY is its first L-1 level slices."""
    ext = _ext()
    G = L if mode == 0 else L - 1
    m4 = 4 * d
    g = torch.Generator(device=DEV).manual_seed(77 + mode + B)

    def rn(*s, scale=1.0):
        return (torch.randn(*s, device=DEV, generator=g) * scale).to(BF)
    c = dict(tokens=rn(B, N, d) if mode == 0 else None,
             levels=rn(B, N, L, d), pos=rn(N, d) if mode == 1 else None,
             w1=rn(G * m4, d, scale=0.04), b1=rn(G * m4),
             w2=rn(G * d, m4, scale=0.04), b2=rn(G * d), G=G, m4=m4)
    _, c["Hpre"], c["Hact"], c["td_in"] = ext.grouped_ff_fwd(
        c["tokens"], c["levels"], c["pos"], c["w1"], c["b1"], c["w2"],
        c["b2"], mode)
    c["w1t"] = c["w1"].view(G, m4, d).transpose(1, 2).contiguous()
    c["w2t"] = c["w2"].view(G, d, m4).transpose(1, 2).contiguous()
    return c


@functools.lru_cache(maxsize=None)
def _dmix(B, N, L, d):
    g = torch.Generator(device=DEV).manual_seed(5 + B + L)
    return torch.randn(B, N, L, d, device=DEV, generator=g).to(BF)


def _dmix_lo(B, N, L, d, lo):
    x = _dmix(B, N, L, d).clone()
    x[:, :, :lo] = 0
    return x


def _ff_bwd(c, mode, dY, g_lo, *extra):
    return _ext().grouped_ff_bwd(
        dY, c["tokens"], c["levels"], c["pos"], c["w1"], c["w2"], c["Hpre"],
        c["Hact"], mode, c["w1t"], c["w2t"], c["td_in"], g_lo, *extra)


@pytest.mark.parametrize("shape", [(2, 9, 3, 8), (32, 256, 6, 512)],
                         ids=["generic", "nt5p_nt8p_tn_tr_sk"])
def test_top_down_backward_reads_dmix_in_place(shape):
    B, N, L, d = shape
    c = _ff_case(B, N, L, d, 1)
    G = c["G"]
    for g_lo in (0, 1, G):
        dmix = _dmix_lo(B, N, L, d, g_lo)
        dtd = dmix[:, :, :L - 1].contiguous()
        ref = _ff_bwd(c, 1, dtd, g_lo)
        got = _ff_bwd(c, 1, dmix, g_lo, L * d)
        torch.cuda.synchronize()
        for name, a, b in zip(OUT6, got, ref):
            assert _same(a, b), (shape, g_lo, name)
        if g_lo < G:
            assert got[4].float().abs().sum() > 0       # a live dW2


@pytest.mark.parametrize("shape", [(2, 9, 3, 8), (2, 256, 4, 256)], ids=str)
def test_db2_once(shape):
    ext = _ext()
    B, N, L, d = shape
    bu, td = _ff_case(B, N, L, d, 0), _ff_case(B, N, L, d, 1)
    for g_lo in range(L):
        dmix = _dmix_lo(B, N, L, d, g_lo)
        dtd = dmix[:, :, :L - 1].contiguous()
        # the unchanged ops: the top-down dB2 is the bottom-up one without
        # the top level
        b2_bu = _ff_bwd(bu, 0, dmix, g_lo)[5]
        b2_td = _ff_bwd(td, 1, dtd, g_lo)[5]
        assert _same(b2_td, b2_bu[:(L - 1) * d]), (shape, g_lo)
        # the cone-aware sum equals both; rows below g_lo poisoned: unread
        poisoned = dmix.clone()
        poisoned.view(torch.int16)[:, :, :g_lo] = NAN_BITS
        one_bu, one_td = ext.db2_cone(poisoned, g_lo)
        assert _same(one_bu, b2_bu) and _same(one_td, b2_td), (shape, g_lo)
        assert (_bits(one_bu[:g_lo * d]) == 0).all()
        # handed in ready, it is what the op returns
        got = _ff_bwd(td, 1, dmix, g_lo, L * d, one_td, False)
        for name, a, b in zip(OUT6, got, _ff_bwd(td, 1, dtd, g_lo)):
            assert _same(a, b), (shape, g_lo, name)
        assert got[5].data_ptr() == one_td.data_ptr()
    # g_lo = L: every column dead
    z_bu, z_td = ext.db2_cone(_dmix(B, N, L, d), L)
    assert not _bits(z_bu).any() and not _bits(z_td).any()
    # without a ready dB2 the strided op sums the strided matrix itself
    dmix = _dmix_lo(B, N, L, d, 1)
    got = _ff_bwd(td, 1, dmix, 1, L * d)
    assert _same(got[5], _ff_bwd(bu, 0, dmix, 1)[5][:(L - 1) * d])


def _poison_free_blocks(like, n):
    """Fill n blocks of like's size with NaNs and free them, so the next
    torch.empty of that size starts out poisoned."""
    junk = [torch.full_like(like.view(torch.int16), NAN_BITS)
            for _ in range(n)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("shape", [(2, 9, 3, 8), (2, 256, 4, 256)], ids=str)
def test_no_fill_ops_feed_merge_and_dpos(shape):
    """grouped_ff_bwd / consensus_bwd under no_fill leave their dead slices
    unwritten (here: NaNs); grad_merge and the cone-aware dpos never read
    them and give what the filling ops, add4 and the full dpos give."""
    ext = _ext()
    B, N, L, d = shape
    bu, td = _ff_case(B, N, L, d, 0), _ff_case(B, N, L, d, 1)
    levels = bu["levels"]
    _, probs, rnorm = ext.consensus_fwd(levels, False, None)
    for lo in range(L):
        dmix = _dmix_lo(B, N, L, d, lo)
        dtd = dmix[:, :, :L - 1].contiguous()
        r_bu = _ff_bwd(bu, 0, dmix, lo)
        r_td = _ff_bwd(td, 1, dtd, lo)
        r_at = ext.consensus_bwd(dmix, levels, probs, rnorm, False, None, lo)
        ref = torch.empty_like(dmix)
        ext.add4_into(dmix, r_bu[1], r_td[1], r_at, ref)
        ref_dpos = ext.dpos(r_td[1])

        b2_bu, b2_td = ext.db2_cone(dmix, lo)
        _poison_free_blocks(dmix, 4)
        g_bu = _ff_bwd(bu, 0, dmix, lo, 0, b2_bu, True)
        g_td = _ff_bwd(td, 1, dmix, lo, L * d, b2_td, True)
        g_at = ext.consensus_bwd(dmix, levels, probs, rnorm, False, None,
                                 lo, True)
        got, _ = ext.grad_merge(dmix, g_bu[1], g_td[1], g_at, lo, False,
                                False)
        got_dpos = ext.dpos(g_td[1], lo + 1)
        torch.cuda.synchronize()
        assert _same(got, ref), (shape, lo)
        assert _same(got_dpos, ref_dpos), (shape, lo)
        for i in (0, 2, 3, 4, 5):       # everything but dLevels: unchanged
            assert _same(g_bu[i], r_bu[i]) and _same(g_td[i], r_td[i]), \
                (shape, lo, OUT6[i])
    # no live top-down group: dPos is a plain zero fill
    z = ext.dpos(torch.full_like(_dmix(B, N, L, d).view(torch.int16),
                                 NAN_BITS).view(BF), L)
    assert z.shape == (N, d) and not _bits(z).any()


def test_merged_top_down_call_equals_the_compact_filled_call():
    """The top-down call exactly as the merged backward makes it, dmix read
    in place at row stride L*d, dB2 handed in from db2_cone and no_fill
    set, against the compact-dY call that fills: dLevels over the levels
    [g_lo + 1, L) that the no-fill contract says are written, every weight
    and bias gradient everywhere, for every first live group."""
    ext = _ext()
    B, N, L, d = 2, 256, 4, 256
    td = _ff_case(B, N, L, d, 1)
    for g_lo in range(td["G"] + 1):
        dmix = _dmix_lo(B, N, L, d, g_lo)
        ref = _ff_bwd(td, 1, dmix[:, :, :L - 1].contiguous(), g_lo)
        b2_td = ext.db2_cone(dmix, g_lo)[1]
        _poison_free_blocks(dmix, 4)
        got = _ff_bwd(td, 1, dmix, g_lo, L * d, b2_td, True)
        torch.cuda.synchronize()
        lo, hi = _ranges(g_lo, L)[0][2]       # the top-down range
        assert (lo, hi) == (g_lo + 1, L)
        assert torch.equal(got[1][:, :, lo:hi], ref[1][:, :, lo:hi]), g_lo
        assert _same(got[1][:, :, lo:hi], ref[1][:, :, lo:hi]), g_lo
        for i in (0, 2, 3, 4, 5):
            assert torch.equal(got[i], ref[i]) and _same(got[i], ref[i]), \
                (g_lo, OUT6[i])
        assert got[5].data_ptr() == b2_td.data_ptr()


# ------------------------------ 3. model ------------------------------- #

# image_size == patch_size is the smallest image a model accepts (one
# patch); the 3 x 3 grid adds rows that are no multiple of anything
CFGS = {
    "d64_L3_n1": dict(dim=64, levels=3, image_size=7, patch_size=7),
    "d512_L6_n1": dict(dim=512, levels=6, image_size=7, patch_size=7),
    "d64_L3_n9": dict(dim=64, levels=3, image_size=21, patch_size=7),
    "d512_L6_n9": dict(dim=512, levels=6, image_size=21, patch_size=7),
}
ITERS, GRAD_ITERS = 6, 4


@functools.lru_cache(maxsize=None)
def _model_and_img(name):
    cfg = CFGS[name]
    torch.manual_seed(0)
    m = Glom(**cfg).to(DEV, BF)
    s = cfg["image_size"]
    img = torch.randn(2, 3, s, s, device=DEV).to(BF)
    return m, img


def _both(fn):
    from glom_pytorch_amd import ops
    try:
        ops.set_bwd_merge(True)
        on = fn()
        ops.set_bwd_merge(False)
        off = fn()
    finally:
        ops.set_bwd_merge(True)
    torch.cuda.synchronize()
    return on, off


def _assert_dicts_same(a, b):
    assert set(a) == set(b) and len(b) >= 10
    for n in b:
        assert _same(a[n], b[n]), n


def _eager_grads(name, read="index", lmin="top", passes=1):
    """Image and parameter gradients of a loss on the top level at time
    GRAD_ITERS; `passes` backward passes over one retained graph."""
    from glom_pytorch_amd import ops
    m, img = _model_and_img(name)
    x = img.clone().requires_grad_(True)
    names = [n for n, _ in m.named_parameters()]
    params = [p for _, p in m.named_parameters()]
    traj = m(x, iters=ITERS, return_all=True, grad_iters=GRAD_ITERS,
             loss_level_min=m.levels - 1 if lmin == "top" else lmin)
    at_t = (ops.trajectory_at(traj, GRAD_ITERS) if read == "at"
            else traj[GRAD_ITERS])
    loss = at_t[:, :, -1].float().pow(2).sum()
    out = []
    for i in range(passes):
        gs = torch.autograd.grad(loss, [x] + params, allow_unused=True,
                                 retain_graph=i + 1 < passes)
        out.append({n: g.clone() for n, g in zip(["img"] + names, gs)
                    if g is not None})
    torch.cuda.synchronize()
    return traj.detach().clone(), out


@pytest.mark.parametrize("read", ["index", "at"])
@pytest.mark.parametrize("name", list(CFGS))
def test_eager_gradients_equal_on_and_off(name, read):
    (t1, g1), (t0, g0) = _both(lambda: _eager_grads(name, read))
    assert _same(t1, t0)
    _assert_dicts_same(g1[0], g0[0])
    assert "img" in g0[0] and "init_levels" in g0[0]
    assert g0[0]["bottom_up.net.1.weight"].float().abs().sum() > 0


@pytest.mark.parametrize("name", ["d64_L3_n9", "d512_L6_n1"])
def test_check_mode_runs_the_merged_path(name):
    from glom_pytorch_amd import ops
    ops.set_check_level_cone(True)
    try:
        (_, g1), (_, g0) = _both(lambda: _eager_grads(name, "at"))
    finally:
        ops.set_check_level_cone(False)
    _assert_dicts_same(g1[0], g0[0])


@pytest.mark.parametrize("name", ["d64_L3_n9", "d512_L6_n1"])
def test_two_backward_passes_over_a_retained_graph(name):
    (_, g1), (_, g0) = _both(lambda: _eager_grads(name, "at", passes=2))
    _assert_dicts_same(g1[0], g1[1])
    _assert_dicts_same(g1[0], g0[0])
    _assert_dicts_same(g1[1], g0[1])


@pytest.mark.parametrize("graph_step", [True, False],
                         ids=["captured", "eager_launch"])
@pytest.mark.parametrize("name", list(CFGS))
def test_trainer_steps_equal_on_and_off(name, graph_step):
    from glom_pytorch_amd.parallel.trainer import DenoisingTrainer

    def train():
        cfg = CFGS[name]
        torch.manual_seed(0)
        m = Glom(**cfg).to(DEV, BF)
        tr = DenoisingTrainer(m, lr=1e-3, decode_step=GRAD_ITERS,
                              graph_step=graph_step)
        assert tr.level_cone
        s = cfg["image_size"]
        img = torch.randn(2, 3, s, s, device=DEV).to(BF)
        torch.manual_seed(1)
        losses = [tr.step(img, iters=ITERS) for _ in range(3)]
        torch.cuda.synchronize()
        return (losses, [q.detach().clone() for q in tr._params]
                + [w.clone() for w in tr.master])
    (l1, p1), (l0, p0) = _both(train)
    assert l1 == l0 and all(x == x for x in l1)
    assert len(p1) == len(p0) and len(p0) >= 20
    for a, b in zip(p1, p0):
        assert a.dtype == b.dtype and torch.equal(
            a.view(torch.int16 if a.dtype == BF else torch.int32),
            b.view(torch.int16 if b.dtype == BF else torch.int32))


def test_no_promise_runs_the_unmerged_path():
    """No loss_level_min, a loss that reads two times: TrajectoryFn and the
    unmerged backward, whatever the switch says; checked against the fp32
    eager specification as tests/test_gpu_native.py does (cosine > 0.99 per
    parameter gradient)."""
    from glom_pytorch_amd.ops import functional as Fn
    cfg = CFGS["d64_L3_n9"]
    torch.manual_seed(0)
    m32 = Glom(**cfg).to(DEV)
    m32.force_eager = True
    mbf = Glom(**cfg).to(DEV)
    mbf.load_state_dict(m32.state_dict())
    mbf = mbf.to(BF)
    img = torch.randn(2, 3, 21, 21, device=DEV)

    def grads(model, x):
        model.zero_grad(set_to_none=True)
        traj = model(x, iters=ITERS, return_all=True, grad_iters=GRAD_ITERS)
        if model is mbf:
            assert not hasattr(traj, "_glom_steps")
            assert type(traj.grad_fn).__name__.startswith("TrajectoryFn")
        (traj[GRAD_ITERS].float().pow(2).mean()
         + traj[2][:, :, -1].float().pow(2).mean()).backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in model.named_parameters()
                if p.grad is not None}
    on, off = _both(lambda: grads(mbf, img.to(BF)))
    _assert_dicts_same(on, off)
    ref = grads(m32, img)
    assert set(ref) == set(on)
    for n in ref:
        cos = torch.nn.functional.cosine_similarity(
            ref[n].float().flatten(), on[n].float().flatten(), dim=0).item()
        assert cos > 0.99, (n, cos)
    assert Fn.trajectory_at(torch.arange(6).view(3, 2), 1).tolist() == [2, 3]


def test_carry_guard():
    """dmix_next is handed out once, to the very tensor it was made from."""
    from glom_pytorch_amd.ops.functional import _BwdCarry
    c = _BwdCarry(posz=True)
    dl = torch.zeros(2, 4, 3, 8, device=DEV, dtype=BF)
    dm = torch.ones_like(dl)
    assert c.take(dl, 0) is None                    # nothing kept
    c.put(dl, dm, 1)
    assert c.take(dl.view_as(dl), 1) is dm          # same storage: taken
    assert c.take(dl, 1) is None                    # and only once
    c.put(dl, dm, 1)
    assert c.take(dl + 0, 1) is None                # something was added
    c.put(dl, dm, 1)
    assert c.take(dl, 0) is None                    # cone starts lower
    c.put(dl, dm, 1)
    assert c.take(dl.transpose(0, 1), 1) is None    # other strides


@pytest.mark.parametrize("read", ["index", "at"])
def test_every_step_but_the_last_takes_the_carried_dmix(read, monkeypatch):
    """In a real backward autograd hands dLevels through untouched: all
    steps below the last differentiated one find their dmix ready."""
    from glom_pytorch_amd.ops.functional import _BwdCarry
    hits = []
    take = _BwdCarry.take

    def counting(self, dnew, lo):
        dm = take(self, dnew, lo)
        hits.append(dm is not None)
        return dm
    monkeypatch.setattr(_BwdCarry, "take", counting)
    _eager_grads("d64_L3_n9", read)
    assert hits == [False] + [True] * (GRAD_ITERS - 1)


def test_switch_defaults_on_and_follows_the_environment(monkeypatch):
    from glom_pytorch_amd import ops
    from glom_pytorch_amd.ops import functional as Fn
    assert Fn.BWD_MERGE is True
    m, img = _model_and_img("d64_L3_n9")

    def merged():
        traj = m(img, iters=ITERS, return_all=True, grad_iters=GRAD_ITERS,
                 loss_level_min=2)
        return hasattr(traj, "_glom_steps")
    monkeypatch.delenv("GLOM_NO_BWD_MERGE", raising=False)
    assert merged()
    monkeypatch.setenv("GLOM_NO_BWD_MERGE", "1")
    assert not merged()
    monkeypatch.delenv("GLOM_NO_BWD_MERGE")
    for k, v in (("GLOM_BWD_FORK", "4"), ("GLOM_NO_BWD_STREAMS", "1")):
        monkeypatch.setenv(k, v)
        assert not merged()
        monkeypatch.delenv(k)
    try:
        ops.set_bwd_merge(False)
        assert not merged()
    finally:
        ops.set_bwd_merge(True)
    assert merged()
    torch.cuda.synchronize()
