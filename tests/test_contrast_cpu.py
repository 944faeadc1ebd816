"""Column-contrastive loss: the torch specification against an independent
per-row loop, gradcheck, edge cases, validation, the model helper and the
trainer option (all on the CPU)."""

import math

import pytest
import torch

from conftest import SMALL
from _contrast_util import MODES, make_inputs

import glom_pytorch_amd
from glom_pytorch_amd import Glom, contrast
from glom_pytorch_amd.contrast import column_contrastive_loss


def loop_loss(a, b, temperature, negatives):
    """The definition, row by row in Python floats (fp64): no masks, no
    logsumexp."""
    B, N, D = a.shape
    rows_a = a.reshape(B * N, D).double().tolist()
    rows_b = b.reshape(B * N, D).double().tolist()
    M = B * N

    def rnorm(v):
        return 1.0 / max(math.sqrt(sum(x * x for x in v)), 1e-8)

    ra = [rnorm(v) for v in rows_a]
    rb = [rnorm(v) for v in rows_b]
    total = 0.0
    for i in range(M):
        z, pos = 0.0, None
        for j in range(M):
            if negatives == "other_images" and j != i and j // N == i // N:
                continue
            dot = sum(x * y for x, y in zip(rows_a[i], rows_b[j]))
            s = ra[i] * rb[j] * dot / temperature
            if j == i:
                pos = s
            z += math.exp(s)
        total += math.log(z) - pos
    return total / M


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(3, 9, 64, 0.1), (2, 5, 16, 0.05),
                                   (1, 4, 8, 0.5)])
def test_spec_matches_row_loop(shape, mode):
    B, N, D, T = shape
    a, b = make_inputs(B, N, D, dtype=torch.float64)
    want = loop_loss(a, b, T, mode)
    got = column_contrastive_loss(a, b, T, mode)
    assert got.dtype == torch.float64 and got.shape == ()
    assert abs(got.item() - want) <= 1e-12 * max(1.0, abs(want))
    # fp32 / bf16 inputs compute in fp32 and return fp32
    got32 = column_contrastive_loss(a.float(), b.float(), T, mode)
    assert got32.dtype == torch.float32
    assert abs(got32.item() - want) <= 1e-5


def test_recipe_losses():
    """The input recipe is non-degenerate and the modes differ (fp64 values
    at seed 0 of the smallest shape)."""
    a, b = make_inputs(3, 9, 64)
    oi = column_contrastive_loss(a.double(), b.double(), 0.1, "other_images")
    al = column_contrastive_loss(a.double(), b.double(), 0.1, "all")
    assert round(oi.item(), 2) == 0.54 and round(al.item(), 2) == 1.08


@pytest.mark.parametrize("mode", MODES)
def test_gradcheck(mode):
    a, b = make_inputs(2, 3, 8, dtype=torch.float64)
    a.requires_grad_(True)
    b.requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda x, y: column_contrastive_loss(x, y, 0.1, mode), (a, b))


def test_single_image_is_exactly_zero():
    a, b = make_inputs(1, 7, 16, dtype=torch.float32)
    a.requires_grad_(True)
    loss = column_contrastive_loss(a, b, 0.1, "other_images")
    assert loss.item() == 0.0
    loss.backward()
    assert torch.isfinite(a.grad).all()
    assert column_contrastive_loss(a, b, 0.1, "all").item() > 0.0


def test_symmetric_is_mean_of_both_orders():
    a, b = make_inputs(3, 5, 16, dtype=torch.float64)
    ab = column_contrastive_loss(a, b, 0.2)
    ba = column_contrastive_loss(b, a, 0.2)
    assert ab.item() != ba.item()
    sym = column_contrastive_loss(a, b, 0.2, symmetric=True)
    assert sym.item() == (0.5 * (ab + ba)).item()


def test_zero_rows_are_clamped():
    a, b = make_inputs(2, 3, 8, dtype=torch.float32)
    a[0, 1] = 0.0
    a.requires_grad_(True)
    loss = column_contrastive_loss(a, b, 0.1)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(a.grad).all()


def test_argument_validation():
    a, b = make_inputs(2, 3, 8, dtype=torch.float32)
    with pytest.raises(ValueError):
        column_contrastive_loss(a, b[:, :2])
    with pytest.raises(ValueError):
        column_contrastive_loss(a[0], b[0])
    with pytest.raises(ValueError):
        column_contrastive_loss(a, b, temperature=0.0)
    with pytest.raises(ValueError):
        column_contrastive_loss(a, b, temperature=-1.0)
    with pytest.raises(ValueError):
        column_contrastive_loss(a, b, negatives="same_image")
    with pytest.raises(ValueError):
        column_contrastive_loss(a, b.double())


def test_exports_and_cpu_path_is_not_native():
    assert glom_pytorch_amd.column_contrastive_loss is column_contrastive_loss
    assert glom_pytorch_amd.contrast is contrast
    a, b = make_inputs(2, 3, 8)          # bf16 on the CPU: torch path
    calls = contrast.native_calls()
    assert column_contrastive_loss(a, b).dtype == torch.float32
    assert contrast.native_calls() == calls


def test_model_helper_slices_the_level():
    m = Glom(**SMALL)
    la = torch.randn(2, m.num_patches, m.levels, m.dim)
    lb = la + 0.5 * torch.randn_like(la)
    for level in (-1, 0, 1):
        want = column_contrastive_loss(la[:, :, level], lb[:, :, level],
                                       temperature=0.2, negatives="all")
        got = m.contrastive_loss(la, lb, level=level, temperature=0.2,
                                 negatives="all")
        assert got.item() == want.item()
    assert (m.contrastive_loss(la, lb).item()
            == column_contrastive_loss(la[:, :, -1], lb[:, :, -1]).item())
    assert (m.contrastive_loss(la, lb, level=0).item()
            != m.contrastive_loss(la, lb, level=-1).item())
    with pytest.raises(ValueError):
        m.contrastive_loss(la[0], lb[0])


def _trainer(**kw):
    from glom_pytorch_amd.parallel.trainer import DenoisingTrainer
    torch.manual_seed(0)
    return DenoisingTrainer(Glom(**SMALL), noise_std=0.5, decode_step=2, **kw)


def test_trainer_with_contrast_runs():
    tr = _trainer(contrast_weight=0.5)
    img = torch.randn(2, 3, 32, 32)
    before = [q.detach().clone() for q in tr._params]
    losses = [tr.step(img, iters=3) for _ in range(2)]
    assert all(math.isfinite(l) for l in losses)
    assert any(not torch.equal(x, q) for x, q in zip(before, tr._params))
    # the term is really in the loss: weight 0 gives another value
    plain = _trainer()
    assert plain.step(img, iters=3) != losses[0]


def test_trainer_weight_zero_is_bitwise_the_plain_step():
    img = torch.randn(2, 3, 32, 32)

    def run(**kw):
        tr = _trainer(**kw)
        torch.manual_seed(1)
        losses = [tr.step(img, iters=3) for _ in range(2)]
        return losses, [q.detach().clone() for q in tr._params]

    l0, p0 = run()
    l1, p1 = run(contrast_weight=0.0)
    assert l0 == l1
    for x, y in zip(p0, p1):
        assert torch.equal(x, y)


def test_trainer_rejects_bad_settings_and_micro_batches():
    with pytest.raises(ValueError):
        _trainer(contrast_weight=-1.0)
    with pytest.raises(ValueError):
        _trainer(contrast_negatives="nope")
    tr = _trainer(contrast_weight=0.5, micro_batches=2)
    with pytest.raises(NotImplementedError):
        tr.step(torch.randn(2, 3, 32, 32), iters=3)
