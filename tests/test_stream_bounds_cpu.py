"""The references and bounds of tests/_stream_util.py, tested on the CPU.

Plain torch-f32 emulations of each kernel's contract (bf16 operands, f32
arithmetic in the documented order, one bf16 rounding) must pass the
checkers; each of a set of planted faults must fail them. The faults are
the ones whole-tensor relative norms of 2e-2 (level mix) and 1e-4 (AdamW
masters) let through. The worst err / tol of every bounded check is printed
(profiles/README.md records them).
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _bounds_util import assert_exact, assert_within, int_probe, round_once
from _stream_util import (BF, NEG_ZERO, STEP_STRIDE, U32, adamw_step_ref,
                          clip_scale, colsum_ref, db2_ref, dpos_ref, f32,
                          merge_ranges, merge_ref, merge_tol, mix_bwd_ref,
                          mix_next_ref, mix_ref, nan_like, norm_ref,
                          plant_zeros, poison_outside)

SHAPES = [(1, 1, 2, 8), (2, 9, 3, 24), (3, 7, 5, 72)]


def _to_bf16(x32, trunc=False):
    if not trunc:
        return x32.to(BF)
    bits = x32.contiguous().view(torch.int32) >> 16
    return bits.to(torch.int16).view(BF)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------- the exactness claims ---------------------------- #

def test_division_by_three_and_four_rounds_once():
    """bf16(f32(n / c)) == n / c rounded once to bf16, for every integer
    |n| <= 1024 and for every finite bf16 value, c in {3, 4}."""
    n = torch.arange(-1024, 1025, dtype=torch.float64)
    for c in (3.0, 4.0):
        got = (n.float() / c).to(BF)
        want = round_once(n / c, BF)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        if c == 3.0:                # most of these results do round
            assert int((got.double() != n / c).sum()) == 1452
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    v = v[torch.isfinite(v.float())]
    assert v.numel() == 65536 - 2 * 128
    for c in (3.0, 4.0):
        got = (v.float() / c).to(BF)
        want = round_once(v.double() / c, BF)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# ------------------------------ level mix ------------------------------ #

def _mix_inputs(shape, integer, seed=0):
    B, N, L, d = shape
    g = _gen(seed + L + d)
    if integer:
        mk = lambda *s: int_probe(s, -256, 256, g)
    else:
        mk = lambda *s: torch.randn(*s, generator=g).to(BF)
    prev, bu, cons = mk(B, N, L, d), mk(B, N, L, d), mk(B, N, L, d)
    return prev, bu, mk(B, N, L - 1, d), cons, mk(B, N, d)


def _mix_emulate(prev, bu, td, cons, bu0=None, fault=None):
    """((prev + bu) + cons) (+ td below the top level), / c_l, to bf16."""
    B, N, L, d = prev.shape
    b = bu.float().clone()
    if bu0 is not None and fault != "bu0_ignored":
        b[:, :, 0] = bu0.float()
    v = prev.float() + b + cons.float()
    tdp = F.pad(td.float(), (0, 0, 0, 1))
    has_td = torch.arange(L).view(1, 1, L, 1) < L - 1
    if fault == "td_top":
        tdp[:, :, L - 1] = td.float()[:, :, L - 2]
        has_td = torch.ones_like(has_td)
    v = torch.where(has_td, v + tdp, v)
    c = torch.full((1, 1, L, 1), 4.0)
    c[:, :, L - 1] = 4.0 if fault == "c_top" else 3.0
    c = c.expand(B, N, L, d)
    if fault == "pow2_d":
        d2 = 1 << (d - 1).bit_length()
        lvl = (torch.arange(prev.numel()) // d2) % L
        c = torch.where(lvl < L - 1, 4.0, 3.0).view(B, N, L, d)
    return _to_bf16(v / c, trunc=fault == "trunc")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mix_emulation_passes(shape):
    for use_bu0 in (False, True):
        prev, bu, td, cons, bu0 = _mix_inputs(shape, True)
        if use_bu0:
            bu[:, :, 0] = nan_like(bu[:, :, 0])
        ref, _ = mix_ref(prev, bu, td, cons, bu0 if use_bu0 else None)
        out = _mix_emulate(prev, bu, td, cons, bu0 if use_bu0 else None)
        assert_exact(out, ref, "mix int")
        prev, bu, td, cons, bu0 = _mix_inputs(shape, False)
        ref, tol = mix_ref(prev, bu, td, cons, bu0 if use_bu0 else None)
        out = _mix_emulate(prev, bu, td, cons, bu0 if use_bu0 else None)
        r = assert_within(out, ref, tol, "mix randn")
        print("cpu mix fwd %s bu0=%d err/tol %.3f" % (shape, use_bu0, r))
        assert r <= 1


def test_mix_bound_over_many_samples():
    """2^20 random samples against the real-operand bound."""
    prev, bu, td, cons, _ = _mix_inputs((64, 64, 4, 64), False, seed=5)
    ref, tol = mix_ref(prev, bu, td, cons)
    r = assert_within(_mix_emulate(prev, bu, td, cons), ref, tol)
    print("cpu mix fwd 2^20 samples err/tol %.4f" % r)
    assert r <= 1


@pytest.mark.parametrize("fault", ["c_top", "td_top", "pow2_d", "trunc",
                                   "bu0_ignored"])
def test_mix_faults_fail(fault):
    shape = (2, 9, 3, 24)
    for integer in (True, False):
        prev, bu, td, cons, bu0 = _mix_inputs(shape, integer)
        use = bu0 if fault == "bu0_ignored" else None
        if use is not None:
            bu[:, :, 0] = nan_like(bu[:, :, 0])
        ref, tol = mix_ref(prev, bu, td, cons, use)
        bad = _mix_emulate(prev, bu, td, cons, use, fault)
        with pytest.raises(AssertionError):
            if integer:
                assert_exact(bad, ref)
            else:
                assert_within(bad, ref, tol)


def test_mix_next_reference():
    prev, bu, td, cons, _ = _mix_inputs((2, 9, 3, 64), True)
    out = _mix_emulate(prev, bu, td, cons)
    out[1, 4, 2] = 0.0                       # an all-zero row
    pos = int_probe((9, 64), -256, 256, _gen(1))
    td64, rn64, rn_tol = mix_next_ref(out, pos)
    td_next = (out.float()[:, :, 1:] + pos.float().view(1, 9, 1, 64)).to(BF)
    assert_exact(td_next, td64, "td_next")
    ss = out.float().pow(2).sum(-1)
    rn = (1.0 / ss.sqrt().clamp_min(1e-12)).permute(0, 2, 1).contiguous()
    r = assert_within(rn, rn64, rn_tol, "rn_next")
    print("cpu rn_next err/tol %.3f" % r)
    assert rn[1, 2, 4] == f32(1.0 / f32(1e-12))
    with pytest.raises(AssertionError):      # norms laid out (B,N,L)
        assert_within(rn.permute(0, 2, 1).reshape(rn.shape), rn64, rn_tol)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_mix_bwd_emulation_and_faults(shape):
    B, N, L, d = shape
    for dout in (int_probe(shape, -256, 256, _gen(2)),
                 torch.randn(shape, generator=_gen(3)).to(BF)):
        dmix64, dtd64 = mix_bwd_ref(dout)
        c = torch.full((1, 1, L, 1), 4.0)
        c[:, :, L - 1] = 3.0
        dmix = (dout.float() / c).to(BF)
        assert_exact(dmix, dmix64, "dmix")
        assert_exact(dmix[:, :, :L - 1], dtd64, "dtd")
        if dout.numel() < 100:       # 16 elements can all round downward
            continue
        with pytest.raises(AssertionError):
            assert_exact((dout.float() / 4.0).to(BF), dmix64)
        with pytest.raises(AssertionError):
            assert_exact(_to_bf16(dout.float() / c, trunc=True), dmix64)


# ------------------------------- merge --------------------------------- #

def _merge_inputs(shape, integer):
    g = _gen(11 + shape[2] + shape[3])
    if integer:
        xs = [int_probe(shape, -256, 256, g) for _ in range(4)]
    else:
        xs = [torch.randn(shape, generator=g).to(BF) for _ in range(4)]
    return plant_zeros(xs, g)


def _merge_emulate(xs, lo, posz, fault=None):
    L = xs[0].shape[2]
    ranges, first = merge_ranges(lo, L)
    if fault == "range_off":                 # top-down read one level low
        ranges = (ranges[0], ranges[1], (max(lo, 0), L), ranges[3])
    lev = torch.arange(L).view(1, 1, L, 1)
    v = None
    for x, (r0, r1) in zip(xs, ranges):
        t = torch.where(((lev >= r0) & (lev < r1)).expand_as(x), x.float(),
                        torch.zeros(()))
        v = t if v is None else v + t
    out = v.to(BF)
    if posz and fault != "neg_zero":
        bits = out.view(torch.int16)
        out = torch.where(bits == NEG_ZERO, torch.zeros_like(bits),
                          bits).view(BF)
    out = torch.where((lev < first).expand_as(out), torch.zeros((), dtype=BF),
                      out)
    c = torch.full((1, 1, L, 1), 4.0)
    c[:, :, L - 1] = 3.0
    return out, (out.float() / c).to(BF)


@pytest.mark.parametrize("shape", [(1, 9, 2, 8), (2, 9, 3, 24)], ids=str)
def test_merge_emulation_passes(shape):
    L = shape[2]
    worst = 0.0
    for integer in (True, False):
        xs = _merge_inputs(shape, integer)
        for lo in range(L + 1):
            for posz in (False, True):
                out, nxt = _merge_emulate(poison_outside(xs, lo, L), lo, posz)
                tot, nxt64, S, first = merge_ref(
                    poison_outside(xs, lo, L), lo, posz)
                if integer:
                    assert_exact(out, tot, "merge out")
                    assert_exact(nxt[:, :, first:], nxt64[:, :, first:],
                                 "merge next")
                else:
                    worst = max(worst, assert_within(
                        out, tot, merge_tol(tot, S), "merge out"))
                    assert_exact(nxt[:, :, first:],
                                 mix_bwd_ref(out)[0][:, :, first:],
                                 "merge next from out")
    print("cpu merge %s err/tol %.3f" % (shape, worst))
    # the planted all -0 positions give -0 where nothing adds +0
    xs = _merge_inputs((2, 9, 3, 24), True)
    out, _ = _merge_emulate(xs, 0, False)
    assert (out.view(torch.int16) == NEG_ZERO).any()
    tot = merge_ref(xs, 0, True)[0]
    assert not (round_once(tot, BF).view(torch.int16) == NEG_ZERO).any()


@pytest.mark.parametrize("fault,posz", [("range_off", False),
                                        ("neg_zero", True)])
def test_merge_faults_fail(fault, posz):
    shape, lo = (2, 9, 3, 24), 1
    xs = _merge_inputs(shape, True)
    if fault == "neg_zero":
        lo = 0
    pz = poison_outside(xs, lo, 3)
    tot, nxt64, _, first = merge_ref(pz, lo, posz)
    out, nxt = _merge_emulate(pz, lo, posz, fault)
    with pytest.raises(AssertionError):
        assert_exact(out, tot)
    with pytest.raises(AssertionError):
        assert_exact(nxt[:, :, first:], nxt64[:, :, first:])


# ----------------------------- reductions ------------------------------ #

def _colsum_emulate(x, fault=None):
    """The two-stage column sum: row chunks of ceil(M / RB) rows, RB =
    min(ceil(M / 64), 256), summed in f32 in chunk order."""
    M, C = x.shape
    RB = min(-(-M // 64), 256)
    chunk = -(-M // RB)
    parts = [x[r:r + chunk].float().sum(0) for r in range(0, M, chunk)]
    if fault == "last_chunk":
        parts = parts[:-1] or [torch.zeros(C)]
    acc = torch.zeros(C)
    for p in parts:
        acc = acc + p
    out = acc.to(BF)
    if fault == "shift8":
        out[8:16] = out[16:24].clone()
    return out


@pytest.mark.parametrize("M,C", [(1, 72), (65, 72), (1025, 72), (1025, 588),
                                 (16385, 24)])
def test_colsum_emulation_and_faults(M, C):
    x = int_probe((M, C), -8, 8, _gen(M + C))
    ref, _ = colsum_ref(x)
    assert_exact(_colsum_emulate(x), ref, "colsum int")
    xr = torch.randn(M, C, generator=_gen(M)).to(BF)
    rr, tol = colsum_ref(xr)
    r = assert_within(_colsum_emulate(xr), rr, tol, "colsum randn")
    print("cpu colsum (%d, %d) err/tol %.3f" % (M, C, r))
    for fault in ("last_chunk", "shift8"):
        with pytest.raises(AssertionError):
            assert_exact(_colsum_emulate(x, fault), ref)
        if M > 1025:     # five rows of 16385 are inside gemm_tol(K = M):
            continue     # there the integer probe is the check
        with pytest.raises(AssertionError):
            assert_within(_colsum_emulate(xr, fault), rr, tol)


def test_db2_and_dpos_references_and_faults():
    B, N, L, d = 2, 33, 3, 24
    x = int_probe((B, N, L, d), -8, 8, _gen(4))
    for lo in range(L + 1):
        p = x.clone()
        p[:, :, :lo] = nan_like(p[:, :, :lo])
        bu64, td64, _ = db2_ref(p, lo)
        live = x.float().clone()
        live[:, :, :lo] = 0.0
        got = live.reshape(B * N, L * d).sum(0).to(BF)
        assert_exact(got, bu64, "db2 bu")
        assert_exact(got[:(L - 1) * d], td64, "db2 td")
        if lo:
            assert not bu64[:lo * d].any()
            # dead columns that hold the sum of what was there
            with pytest.raises(AssertionError):
                assert_exact(x.float().reshape(B * N, L * d).sum(0).to(BF),
                             bu64)
    for l0 in range(1, L + 1):
        p = x.clone()
        p[:, :, :l0] = nan_like(p[:, :, :l0])
        ref, _ = dpos_ref(p, l0)
        got = x.float()[:, :, l0:].sum((0, 2)).to(BF)
        assert_exact(got, ref, "dpos")
        assert ref.shape == (N, d)
        if l0 == L:
            assert not ref.any()
        with pytest.raises(AssertionError):      # starts one level low
            assert_exact(x.float()[:, :, l0 - 1:].sum((0, 2)).to(BF), ref)


# -------------------------------- AdamW -------------------------------- #

HYP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8)


def _fma32(a, b, c):
    """f32 fma through fp64: the product of two f32 values is exact in
    fp64; the sum is rounded to fp64 and then to f32."""
    return (a.double() * b.double() + c.double()).float()


def _adamw_emulate(g, m1, m2, p, wd, t, max_norm, norm, fault=None,
                   lr=HYP["lr"], b1=HYP["b1"], b2=HYP["b2"], eps=HYP["eps"]):
    """The fused step's contract in f32: clip scale from the norm, the two
    moment fmas on the scaled gradient, pow-based bias corrections (numpy's
    fp32 powf), decay as one fma, update, bf16 copy."""
    one = np.float32(1.0)
    lr, b1, b2, eps, wd = (np.float32(x) for x in (lr, b1, b2, eps, wd))
    T = lambda x: torch.tensor(float(x), dtype=torch.float32)
    scale = one
    if max_norm > 0:
        scale = min(one, np.float32(max_norm)
                    / (np.float32(norm) + np.float32(1e-6)))
    tt = np.float32(t - 1 if fault == "t_minus_1" else t)
    bc1 = one - np.power(b1, tt)
    bc2 = one if fault == "no_bc2" else one - np.power(b2, tt)
    step_size, inv_bc2 = T(lr / bc1), T(one / bc2)
    decay = T(np.float32(1.0 - float(lr) * float(wd)))
    gs = g.float() * (one if fault == "clip_m" else T(scale))
    if fault == "l2_wd":
        gs, decay = gs + T(wd) * p, T(1.0)
    m = _fma32(T(b1), m1, T(one - b1) * gs)
    v = _fma32(T(b2), m2, T(one - b2) * gs * gs)
    if fault == "clip_m":
        m = m * T(scale)
    pn = p * decay
    if fault == "eps_in_sqrt":
        pn = pn - step_size * m / torch.sqrt(v * inv_bc2 + T(eps))
    else:
        pn = pn - step_size * m / (torch.sqrt(v * inv_bc2) + T(eps))
    if fault == "second_pass":
        m[STEP_STRIDE:], v[STEP_STRIDE:] = m1[STEP_STRIDE:], m2[STEP_STRIDE:]
        pn[STEP_STRIDE:] = p[STEP_STRIDE:]
    return m, v, pn


def _norm_emulate(grads):
    s = torch.zeros((), dtype=torch.float32)
    for g in grads:
        s = s + g.float().pow(2).sum()
    return float(s.sqrt())


def _state(n, t, gscale, seed):
    """A state as t - 1 steps would leave it (m ~ g, v ~ g^2 (1 - b2^(t-1)))
    and a gradient, with planted exact zeros."""
    g = _gen(seed)
    grad = (torch.randn(n, generator=g) * gscale).to(BF)
    grad[::97] = 0.0
    m1 = torch.randn(n, generator=g) * gscale * (0.0 if t == 1 else 0.3)
    m2 = (torch.randn(n, generator=g) * gscale).pow(2) \
        * (1 - 0.999 ** (t - 1))
    m2[::194] = 0.0
    p = torch.randn(n, generator=g)
    return grad, m1, m2, p


def _check_adamw(got, g, m1, m2, p, wd, t, max_norm, norm):
    scale = clip_scale(norm, max_norm)
    ref, tol = adamw_step_ref(g, m1, m2, p, wd=wd, t=t, scale=scale,
                              e_scale=3 * U32 if max_norm > 0 else 0.0, **HYP)
    return [assert_within(a, r, tl, w)
            for a, r, tl, w in zip(got, ref, tol, ("exp_avg", "exp_avg_sq",
                                                   "master"))]


def test_adamw_emulation_within_bound():
    worst = [0.0, 0.0, 0.0]
    for t in (1, 2, 3, 10, 100, 1000, 100000):
        for gscale in (1e-8, 3.0, 1e3):
            g, m1, m2, p = _state(4096, t, gscale, seed=t % 89)
            true_norm, _ = norm_ref([g])
            for max_norm in (0.0, true_norm * 0.0123):
                norm = _norm_emulate([g])
                got = _adamw_emulate(g, m1, m2, p, 1e-2, t, max_norm, norm)
                r = _check_adamw(got, g, m1, m2, p, 1e-2, t, max_norm, norm)
                worst = [max(a, b) for a, b in zip(worst, r)]
    print("cpu adamw err/tol: exp_avg %.3f exp_avg_sq %.3f master %.3f"
          % tuple(worst))
    assert max(worst) <= 1


def test_norm_bound():
    gs = [(torch.randn(n, generator=_gen(n)) * 3).to(BF)
          for n in (3, 2880, 2 * STEP_STRIDE + 777)]
    ref, tol = norm_ref(gs)
    got = _norm_emulate(gs)
    print("cpu norm err/tol %.3f" % (abs(got - ref) / tol))
    assert abs(got - ref) <= tol
    # a norm that misses the second grid-stride pass of the largest tensor
    short = _norm_emulate(gs[:2] + [gs[2][:262144]])
    assert abs(short - ref) > tol


@pytest.mark.parametrize("fault,t,gscale,clip", [
    ("eps_in_sqrt", 10, 1e-8, 0.0),
    ("no_bc2", 10, 3.0, 0.0),
    ("l2_wd", 10, 3.0, 0.0),
    ("clip_m", 10, 3.0, 0.0123),
    ("t_minus_1", 10, 3.0, 0.0),
    ("t_minus_1", 1000, 3.0, 0.0),
])
def test_adamw_faults_fail(fault, t, gscale, clip):
    g, m1, m2, p = _state(4096, t, gscale, seed=1)
    norm = _norm_emulate([g])
    max_norm = norm * clip
    good = _adamw_emulate(g, m1, m2, p, 1e-2, t, max_norm, norm)
    _check_adamw(good, g, m1, m2, p, 1e-2, t, max_norm, norm)
    bad = _adamw_emulate(g, m1, m2, p, 1e-2, t, max_norm, norm, fault)
    with pytest.raises(AssertionError):
        _check_adamw(bad, g, m1, m2, p, 1e-2, t, max_norm, norm)


def test_adamw_second_pass_untouched_fails():
    n = 2 * STEP_STRIDE + 777
    g, m1, m2, p = _state(n, 10, 3.0, seed=2)
    bad = _adamw_emulate(g, m1, m2, p, 1e-2, 10, 0.0, 0.0, "second_pass")
    with pytest.raises(AssertionError) as e:
        _check_adamw(bad, g, m1, m2, p, 1e-2, 10, 0.0, 0.0)
    assert "%d of %d" % (n - STEP_STRIDE, n) in str(e.value)


def test_adamw_neighbours_weight_decay_fails():
    wds = [0.0, 0.1]
    states = [_state(2880, 10, 3.0, seed=s) for s in (3, 4)]
    for i, (g, m1, m2, p) in enumerate(states):
        good = _adamw_emulate(g, m1, m2, p, wds[i], 10, 0.0, 0.0)
        _check_adamw(good, g, m1, m2, p, wds[i], 10, 0.0, 0.0)
        bad = _adamw_emulate(g, m1, m2, p, wds[1 - i], 10, 0.0, 0.0)
        with pytest.raises(AssertionError):
            _check_adamw(bad, g, m1, m2, p, wds[i], 10, 0.0, 0.0)


def test_adamw_chained_tolerance_tracks_torch():
    """Five f32 steps against torch.optim.AdamW on fp64 clones, with the
    tolerance accumulated step by step (d_in of adamw_step_ref); the
    reference itself must reproduce torch's fp64 state."""
    n, steps, max_norm = 2880, 5, 1.0
    gen = _gen(7)
    p32 = torch.randn(n, generator=gen)
    grads = [(torch.randn(n, generator=gen) * 3).to(BF) for _ in range(steps)]
    tp = p32.double().clone().requires_grad_(True)
    topt = torch.optim.AdamW([tp], lr=f32(HYP["lr"]),
                             betas=(f32(HYP["b1"]), f32(HYP["b2"])),
                             eps=f32(HYP["eps"]), weight_decay=f32(1e-2))
    m, v, p = torch.zeros(n), torch.zeros(n), p32.clone()
    rm, rv, rp = m.double(), v.double(), p.double()
    d_in = None
    for t, g in enumerate(grads, 1):
        norm = _norm_emulate([g])
        m, v, p = _adamw_emulate(g, m, v, p, 1e-2, t, max_norm, norm)
        norm64, norm_tol = norm_ref([g])
        (rm, rv, rp), d_in = adamw_step_ref(
            g, rm, rv, rp, wd=1e-2, t=t, scale=clip_scale(norm64, max_norm),
            e_scale=3 * U32 + norm_tol / norm64, d_in=d_in, **HYP)
        tp.grad = g.double()
        torch.nn.utils.clip_grad_norm_([tp], f32(max_norm))
        topt.step()
    st = topt.state[tp]
    for a, b in ((rm, st["exp_avg"]), (rv, st["exp_avg_sq"]),
                 (rp, tp.detach())):
        assert ((a - b).abs() <= 1e-13 * b.abs().max()).all()
    r = [assert_within(a, b, tl) for a, b, tl in zip((m, v, p), (rm, rv, rp),
                                                     d_in)]
    print("cpu adamw 5 chained steps err/tol %.3f %.3f %.3f" % tuple(r))
