"""Column-contrastive loss on the gfx950 HIP path: forward and backward
against fp64 autograd of the specification, strided inputs, determinism,
bounded memory, hipGraph capture, dispatch, and the trainer option."""

import pytest
import torch

from conftest import SMALL
from _contrast_util import (MODES, SHAPE_IDS, SHAPES, TILE_ALIGNED,
                            emulate_native_grads, make_inputs, reference64,
                            rel_err)

from glom_pytorch_amd import Glom, contrast
from glom_pytorch_amd.contrast import column_contrastive_loss

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"

_cache = {}


def _case(i, mode):
    """Inputs, fp64 loss / gradients and the emulation's errors, once."""
    key = (i, mode)
    if key not in _cache:
        B, N, D, T = SHAPES[i]
        a, b = make_inputs(B, N, D)
        loss64, ga64, gb64 = reference64(a, b, T, mode)
        ea, eb = emulate_native_grads(a, b, T, mode)
        _cache[key] = (a, b, loss64, ga64, gb64,
                       rel_err(ea, ga64), rel_err(eb, gb64))
    return _cache[key]


def _launches():
    from glom_pytorch_amd.ops import _load_extension
    return tuple(_load_extension().nce_launch_counts())   # (fast, generic)


def _fwd_bwd(a, b, T, mode):
    a = a.detach().requires_grad_(True)
    b = b.detach().requires_grad_(True)
    loss = column_contrastive_loss(a, b, T, mode)
    loss.backward()
    return loss.detach(), a.grad, b.grad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPE_IDS)
def test_forward_parity(i, mode):
    B, N, D, T = SHAPES[i]
    a, b, loss64 = _case(i, mode)[:3]
    calls, (fast, generic) = contrast.native_calls(), _launches()
    with torch.no_grad():
        loss = column_contrastive_loss(a.to(DEV), b.to(DEV), T, mode)
    assert contrast.native_calls() == calls + 1
    assert loss.dtype == torch.float32 and loss.shape == ()
    fast2, generic2 = _launches()
    if TILE_ALIGNED[i]:
        assert (fast2, generic2) == (fast + 1, generic), "fast kernel not used"
    else:
        assert (fast2, generic2) == (fast, generic + 1)
    bound = D * 2.0 ** -23 / T
    err = abs(loss.item() - loss64)
    print(f"loss {loss.item():.6f} fp64 {loss64:.6f} err {err:.3e} "
          f"(bound {bound:.3e})")
    assert err <= bound


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPE_IDS)
def test_backward_parity(i, mode):
    """Measured (native, emulation) error pairs: profiles/README.md."""
    B, N, D, T = SHAPES[i]
    a, b, _, ga64, gb64, emu_a, emu_b = _case(i, mode)
    fast, generic = _launches()
    _, ga, gb = _fwd_bwd(a.to(DEV), b.to(DEV), T, mode)
    fast2, generic2 = _launches()
    if TILE_ALIGNED[i]:     # forward + one recompute per side
        assert (fast2, generic2) == (fast + 3, generic)
    assert ga.dtype == torch.bfloat16 and ga.shape == (B, N, D)
    assert ga.is_contiguous() and gb.is_contiguous()
    err_a, err_b = rel_err(ga.cpu(), ga64), rel_err(gb.cpu(), gb64)
    print(f"dA native {err_a:.3e} emulation {emu_a:.3e}; "
          f"dB native {err_b:.3e} emulation {emu_b:.3e}")
    assert err_a <= 2 * emu_a
    assert err_b <= 2 * emu_b


def test_upstream_gradient_scales():
    B, N, D, T = SHAPES[0]
    a, b = _case(0, "other_images")[:2]
    _, ga, gb = _fwd_bwd(a.to(DEV), b.to(DEV), T, "other_images")
    a2 = a.to(DEV).requires_grad_(True)
    (column_contrastive_loss(a2, b.to(DEV), T) * 4.0).backward()
    assert torch.equal(a2.grad, (ga.float() * 4.0).bfloat16())


@pytest.mark.parametrize("mode", MODES)
def test_strided_inputs_same_bits(mode):
    """Level slices of a trajectory are read in place."""
    B, N, D, T = 4, 64, 64, 0.1
    a, b = make_inputs(B, N, D)
    traj = torch.randn(3, B, N, 2, D, device=DEV).bfloat16()
    traj2 = torch.randn(3, B, N, 2, D, device=DEV).bfloat16()
    traj[1, :, :, 1] = a.to(DEV)
    traj2[2, :, :, 0] = b.to(DEV)
    sa, sb = traj[1, :, :, 1], traj2[2, :, :, 0]
    assert not sa.is_contiguous()
    l1, ga1, gb1 = _fwd_bwd(sa, sb, T, mode)
    l2, ga2, gb2 = _fwd_bwd(sa.clone(), sb.clone(), T, mode)
    assert torch.equal(l1, l2)
    assert torch.equal(ga1, ga2) and torch.equal(gb1, gb2)
    # a slice that is not 16-byte aligned is cloned, same bits again
    pad = torch.zeros(B * N * D + 4, device=DEV, dtype=torch.bfloat16)
    odd = pad[4:].view(B, N, D)
    odd.copy_(sa)
    assert odd.data_ptr() % 16 != 0
    l3, ga3, _ = _fwd_bwd(odd, sb, T, mode)
    assert torch.equal(l1, l3) and torch.equal(ga1, ga3)


@pytest.mark.parametrize("i", [0, 3], ids=[SHAPE_IDS[0], SHAPE_IDS[3]])
def test_bitwise_deterministic(i):
    B, N, D, T = SHAPES[i]
    a, b = _case(i, "other_images")[:2]
    a, b = a.to(DEV), b.to(DEV)
    first = _fwd_bwd(a, b, T, "other_images")
    for _ in range(4):
        again = _fwd_bwd(a, b, T, "other_images")
        for x, y in zip(first, again):
            assert torch.equal(x, y)


def test_no_logit_matrix():
    """M = 8192: one bf16 logit matrix would be 128 MiB."""
    B, N, D = 32, 256, 64
    a, b = make_inputs(B, N, D)
    a, b = a.to(DEV), b.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, ga, gb = _fwd_bwd(a, b, 0.1, "other_images")
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise {rise / 2**20:.1f} MiB")
    assert torch.isfinite(loss) and torch.isfinite(ga.float()).all()
    assert rise < 128 * 2 ** 20


def test_graph_capture_replay():
    B, N, D, T = SHAPES[1]
    a, b = _case(1, "other_images")[:2]
    a2, b2 = make_inputs(B, N, D, seed=1)
    ref = _fwd_bwd(a2.to(DEV), b2.to(DEV), T, "other_images")

    sa = a.to(DEV).requires_grad_(True)
    sb = b.to(DEV).requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        column_contrastive_loss(sa, sb, T).backward()      # warmup
    torch.cuda.current_stream().wait_stream(s)
    sa.grad = sb.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = column_contrastive_loss(sa, sb, T)
        loss.backward()
    with torch.no_grad():
        sa.copy_(a2.to(DEV))
        sb.copy_(b2.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), ref[0])
    assert torch.equal(sa.grad, ref[1]) and torch.equal(sb.grad, ref[2])


def test_fallbacks_take_torch_path(monkeypatch):
    B, N, D, T = SHAPES[0]
    a, b, loss64 = _case(0, "other_images")[:3]
    a, b = a.to(DEV), b.to(DEV)
    calls = contrast.native_calls()
    low = column_contrastive_loss(a, b, 0.01)
    f32 = column_contrastive_loss(a.float(), b.float(), T)
    monkeypatch.setenv("GLOM_FORCE_EAGER", "1")
    forced = column_contrastive_loss(a, b, T)
    monkeypatch.delenv("GLOM_FORCE_EAGER")
    assert contrast.native_calls() == calls
    assert torch.isfinite(low)
    assert abs(f32.item() - loss64) < 1e-5
    assert abs(forced.item() - loss64) < 1e-5
    column_contrastive_loss(a, b, T)
    assert contrast.native_calls() == calls + 1


# ------------------------------ trainer -------------------------------- #

def _cos(a, b):
    a, b = a.detach().float().flatten(), b.detach().float().flatten()
    return torch.dot(a, b) / (a.norm() * b.norm() + 1e-12)


def _trainer(graph, **kw):
    from glom_pytorch_amd.parallel.trainer import DenoisingTrainer
    torch.manual_seed(0)
    m = Glom(**SMALL).to(DEV, torch.bfloat16)
    return DenoisingTrainer(m, lr=1e-3, noise_std=0.0, graph_step=graph,
                            decode_step=2, **kw)


def test_trainer_graph_step_matches_eager_with_contrast():
    """Same comparison as the plain graphed-step test; noise_std = 0
    removes the RNG."""
    img = torch.randn(2, 3, 32, 32, device=DEV).to(torch.bfloat16)
    te = _trainer(False, contrast_weight=0.5)
    tg = _trainer(True, contrast_weight=0.5)
    tg.model.load_state_dict(te.model.state_dict())
    tg.decoder.load_state_dict(te.decoder.state_dict())
    with torch.no_grad():
        for mw, q in zip(tg.master, tg._params):
            mw.copy_(q.float())
    calls = contrast.native_calls()
    losses_e = [te.step(img, iters=3) for _ in range(4)]
    assert contrast.native_calls() == calls + 4
    losses_g = [tg.step(img, iters=3) for _ in range(4)]
    assert len(tg._graphs) == 1
    entry = next(iter(tg._graphs.values()))
    assert entry is not False, "capture fell back to eager"
    for le, lg in zip(losses_e, losses_g):
        assert abs(le - lg) < 5e-2 * max(1.0, abs(le)), (le, lg)
    for (ne, pe), (ng, pg) in zip(te.model.named_parameters(),
                                  tg.model.named_parameters()):
        assert _cos(pe, pg) > 0.999, (ne, _cos(pe, pg))


def test_trainer_weight_zero_is_bitwise_the_plain_step():
    img = torch.randn(2, 3, 32, 32, device=DEV).to(torch.bfloat16)
    from glom_pytorch_amd.parallel.trainer import DenoisingTrainer

    def run(**kw):
        torch.manual_seed(0)
        m = Glom(**SMALL).to(DEV, torch.bfloat16)
        tr = DenoisingTrainer(m, lr=1e-3, graph_step=False, decode_step=2,
                              **kw)
        torch.manual_seed(1)
        losses = [tr.step(img, iters=3) for _ in range(2)]
        return losses, [q.detach().clone() for q in tr._params]

    calls = contrast.native_calls()
    l0, p0 = run()
    l1, p1 = run(contrast_weight=0.0)
    assert contrast.native_calls() == calls
    assert l0 == l1
    for x, y in zip(p0, p1):
        assert torch.equal(x, y)
