"""Level mix and the backward level chain, per element against fp64.

The bitwise kernel-against-kernel tests (test_gpu_bwd_merge.py,
test_gpu_mix_fusion.py, test_gpu_token_hoist.py) pin grad_merge, the
lo-limited mix backward and the fused forward to ``ext.level_mix_fwd``,
``ext.level_mix_bwd`` and ``ext.add4_into``; here those anchors, and the
kernels pinned to them, are compared with the references of
tests/_stream_util.py. Integer probes make every comparison bit-exact
(``assert_exact``, signed zeros included); random reals use the derived
bound of ``mix_ref`` / ``merge_tol``. Every element is checked.

Shapes (B, N, L, d): (1,1,2,8) 16 elements at the minimum L; (2,9,3,24) a d
that is no power of two, under one block; (3,7,5,72) 7560 elements, a
partial last block; (2,16,6,512) the headline L and d, 384 blocks.
"""

import functools

import pytest
import torch

from _bounds_util import assert_exact, assert_within, int_probe
from _stream_util import (BF, NEG_ZERO, merge_ref, merge_tol, mix_bwd_ref,
                          mix_next_ref, mix_ref, nan_like, plant_zeros,
                          poison_outside)

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"
SHAPES = [(1, 1, 2, 8), (2, 9, 3, 24), (3, 7, 5, 72), (2, 16, 6, 512)]


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _mix_inputs(shape, integer):
    B, N, L, d = shape
    g = _gen(3 + L + d + integer)
    if integer:
        mk = lambda *s: int_probe(s, -256, 256, g)
    else:
        mk = lambda *s: torch.randn(*s, device=DEV, generator=g).to(BF)
    return (mk(B, N, L, d), mk(B, N, L, d), mk(B, N, L - 1, d),
            mk(B, N, L, d), mk(B, N, d))


def _poison_free_blocks(like, n):
    """Fill n blocks of like's size with NaNs and free them, so the next
    torch.empty of that size starts out poisoned."""
    junk = [nan_like(like) for _ in range(n)]
    torch.cuda.synchronize()
    del junk


# ------------------------------ forward -------------------------------- #

@pytest.mark.parametrize("integer", [True, False], ids=["int", "randn"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_level_mix_fwd(shape, integer):
    ext = _ext()
    prev, bu, td, cons, _ = _mix_inputs(shape, integer)
    ref, tol = mix_ref(prev, bu, td, cons)
    out = ext.level_mix_fwd(prev, bu, td, cons)
    if integer:
        assert_exact(out, ref, "mix fwd")
    else:
        print("mix fwd %s err/tol %.3f"
              % (shape, assert_within(out, ref, tol, "mix fwd")))


@pytest.mark.parametrize("form", ["contiguous", "strided"])
@pytest.mark.parametrize("integer", [True, False], ids=["int", "randn"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_level_mix_fwd_bu0(shape, integer, form):
    """Level 0 of the bottom-up term from a separate (B,N,d) row: compact,
    or a view with row stride L*d into another (B,N,L,d) tensor. Slice 0
    of ``bu`` holds NaNs: a read of it shows."""
    ext = _ext()
    B, N, L, d = shape
    prev, bu, td, cons, bu0 = _mix_inputs(shape, integer)
    bu = bu.clone()
    bu[:, :, 0] = nan_like(bu[:, :, 0])
    if form == "strided":
        host = nan_like(bu)
        host[:, :, 0] = bu0
        bu0 = host[:, :, 0]
        assert bu0.stride(1) == L * d
    ref, tol = mix_ref(prev, bu, td, cons, bu0)
    out = ext.level_mix_fwd(prev, bu, td, cons, None, 0, bu0)
    if integer:
        assert_exact(out, ref, "mix fwd bu0")
    else:
        print("mix fwd bu0 %s %s err/tol %.3f"
              % (shape, form, assert_within(out, ref, tol, "mix fwd bu0")))


@pytest.mark.parametrize("shape", [(1, 3, 2, 512), (2, 9, 3, 512)], ids=str)
def test_level_mix_fwd_next(shape):
    """The fused forward at d = 512: out and td_next = bf16(out + pos)
    exact on integer probes, rn_next within (d + 4) * 2^-24 relative of
    fp64 computed from the stored out; one all-zero row clamps to 1e12."""
    ext = _ext()
    B, N, L, d = shape
    prev, bu, td, cons, bu0 = (t.clone() for t in _mix_inputs(shape, True))
    for t in (prev, bu, cons):
        t[B - 1, N - 1, L - 1] = 0.0            # top level: no td there
    pos = int_probe((N, d), -256, 256, _gen(9))
    ref, _ = mix_ref(prev, bu, td, cons)
    out, td_next, rn_next = ext.level_mix_fwd_next(prev, bu, td, cons, None,
                                                   0, None, pos)
    assert td_next.shape == (B, N, L - 1, d) and rn_next.shape == (B, L, N)
    assert_exact(out, ref, "out")
    td64, rn64, rn_tol = mix_next_ref(out, pos)
    assert_exact(td_next, td64, "td_next")
    print("rn_next %s err/tol %.3f"
          % (shape, assert_within(rn_next, rn64, rn_tol, "rn_next")))
    assert rn_next[B - 1, L - 1, N - 1].item() == pytest.approx(1e12,
                                                                rel=1e-6)
    # with bu0, and on real operands
    bu_p = bu.clone()
    bu_p[:, :, 0] = nan_like(bu_p[:, :, 0])
    out0 = ext.level_mix_fwd_next(prev, bu_p, td, cons, None, 0, bu0, pos)[0]
    assert_exact(out0, mix_ref(prev, bu_p, td, cons, bu0)[0], "out bu0")
    prev, bu, td, cons, _ = _mix_inputs(shape, False)
    pos = torch.randn(N, d, device=DEV, generator=_gen(10)).to(BF)
    ref, tol = mix_ref(prev, bu, td, cons)
    out, td_next, rn_next = ext.level_mix_fwd_next(prev, bu, td, cons, None,
                                                   0, None, pos)
    r = assert_within(out, ref, tol, "out randn")
    td64, rn64, rn_tol = mix_next_ref(out, pos)
    # one f32 add of two bf16 values, one bf16 rounding
    r2 = assert_within(td_next, td64, 2.0 ** -8 * td64.abs()
                       + 2.0 ** -24 * td64.abs(), "td_next randn")
    r3 = assert_within(rn_next, rn64, rn_tol, "rn_next randn")
    print("mix next randn %s err/tol out %.3f td_next %.3f rn %.3f"
          % (shape, r, r2, r3))


# ------------------------------ backward ------------------------------- #

@pytest.mark.parametrize("integer", [True, False], ids=["int", "randn"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_level_mix_bwd(shape, integer):
    """dmix and dtd on the full path; the live levels of the lo-limited
    path, written into poisoned memory, for every lo. Exact for real
    operands too: one divide by 3 or 4 rounds once (_stream_util)."""
    ext = _ext()
    B, N, L, d = shape
    dout = _mix_inputs(shape, integer)[0]
    dmix64, dtd64 = mix_bwd_ref(dout)
    dmix, dtd = ext.level_mix_bwd(dout)
    assert_exact(dmix, dmix64, "dmix")
    assert_exact(dtd, dtd64, "dtd")
    for lo in range(L + 1):
        _poison_free_blocks(dout, 2)
        got, none = ext.level_mix_bwd(dout, lo, False)
        assert none.numel() == 0 and got.shape == dout.shape
        assert_exact(got[:, :, lo:], dmix64[:, :, lo:], "dmix lo=%d" % lo)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_add4_into(shape):
    ext = _ext()
    g = _gen(21 + shape[3])
    xs = plant_zeros([int_probe(shape, -256, 256, g) for _ in range(4)], g)
    out = nan_like(xs[0])
    ext.add4_into(*xs, out)
    ref = xs[0].double() + xs[1].double() + xs[2].double() + xs[3].double()
    assert_exact(out, ref, "add4")
    assert (out.view(torch.int16) == NEG_ZERO).any()     # four -0 give -0
    xr = [torch.randn(shape, device=DEV, generator=g).to(BF)
          for _ in range(4)]
    ext.add4_into(*xr, out)
    ref = sum(x.double() for x in xr)
    S = sum(x.double().abs() for x in xr)
    print("add4 %s err/tol %.3f"
          % (shape, assert_within(out, ref, merge_tol(ref, S), "add4")))


@functools.lru_cache(maxsize=None)
def _merge_inputs(shape, integer):
    g = _gen(11 + shape[2] + shape[3] + integer)
    if integer:
        xs = [int_probe(shape, -256, 256, g) for _ in range(4)]
    else:
        xs = [torch.randn(shape, device=DEV, generator=g).to(BF)
              for _ in range(4)]
    return tuple(plant_zeros(xs, g))


@pytest.mark.parametrize("posz", [False, True], ids=["no_traj", "traj"])
@pytest.mark.parametrize("want_next", [False, True], ids=["plain", "next"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_grad_merge(shape, want_next, posz):
    """grad_merge against merge_ref directly, for every lo; inputs hold
    NaNs outside their ranges and the outputs land in poisoned memory."""
    ext = _ext()
    L = shape[2]
    worst = 0.0
    for integer in (True, False):
        xs = _merge_inputs(shape, integer)
        seen_neg_zero = False
        for lo in range(L + 1):
            poisoned = poison_outside(xs, lo, L)
            tot, nxt64, S, first = merge_ref(poisoned, lo, posz)
            _poison_free_blocks(xs[0], 2)
            got, got_next = ext.grad_merge(*poisoned, lo, posz, want_next)
            what = "%s lo=%d" % (shape, lo)
            if integer:
                assert_exact(got, tot, "merge out " + what)
                seen_neg_zero |= bool(
                    (got.view(torch.int16) == NEG_ZERO).any())
            else:
                worst = max(worst, assert_within(
                    got, tot, merge_tol(tot, S), "merge out " + what))
                # the dead levels are +0 bits, whatever the operands
                assert not got[:, :, :first].view(torch.int16).any()
                # stage by stage: the next dmix from the stored sum
                nxt64 = mix_bwd_ref(got)[0]
            if want_next:
                assert got_next.shape == got.shape
                assert_exact(got_next[:, :, first:], nxt64[:, :, first:],
                             "merge next " + what)
            else:
                assert got_next.numel() == 0
        if integer and posz:
            assert not seen_neg_zero
        elif integer and L >= 3 and xs[0].numel() >= 64:
            assert seen_neg_zero
    print("grad_merge %s err/tol %.3f" % (shape, worst))
