"""Wide (16-byte) register epilogue of the nt5p GEMM, EPI_GELU on
forward-only steps, and the re-blocked k_colsum_fin.

The wide epilogue only re-lays out already-rounded bf16 values, so every
tensor must be bit-identical to the 2-byte epilogue (set_wide_epilogue /
set_wide_epilogue_mode toggle them in-process), and separately correct
against fp32 torch. Modes: 0 narrow, 1 the shipped per-epilogue default,
2 everything wide (= set_wide_epilogue(True)), 3 wide aux loads only.

Shapes are the smallest that reach nt5p (M % 512 == 0, m4 % 256 == 0,
m4 >= 1024, (m4/256)*(M/512)*G >= 96):
  A: B=6 N=256 L=6 d=512  (M=1536, m4=2048; three 4-tile sweeps per column)
  B: B=8 N=256 L=6 d=64, m4=1024 (K=64: nk=1, every k-step ends a tile)
nt8p needs K >= 2048 and (N/256)*(M/256)*G >= 256: the down-projection and
dX of
  C: B=22 N=256 L=6 d=512 (M=5632, m4=2048; grid 2*22*6 = 264)
and, for its aux (EPI_GELUGRAD) path, a dH with K = d >= 2048:
  D: B=2 N=256 L=4 d=2048 (M=512, m4=8192; grid 32*2*4 = 256)
"""

import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU"),
]

DEV = "cuda:0"
BF = torch.bfloat16

# name -> (B, N, L, d, m4)
SHAPES = {"A": (6, 256, 6, 512, 2048), "B": (8, 256, 6, 64, 1024),
          "C": (22, 256, 6, 512, 2048), "D": (2, 256, 4, 2048, 8192)}
# (shape, mode): top-down at shape B has G=5 -> grid 80 < 96, not nt5p
CASES = [("A", 0), ("A", 1), ("B", 0)]


def _ext():
    from glom_pytorch_amd.ops import _load_extension
    return _load_extension()


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-8)).item()


@functools.lru_cache(maxsize=None)
def _inputs(shape, mode):
    B, N, L, d, m4 = SHAPES[shape]
    G = L if mode == 0 else L - 1
    g = torch.Generator(device=DEV).manual_seed(
        1234 + 17 * mode + (0 if shape == "A" else 1))

    def rn(*s, scale=1.0):
        return (torch.randn(*s, device=DEV, generator=g) * scale).to(BF)
    return dict(
        tokens=rn(B, N, d) if mode == 0 else None,
        levels=rn(B, N, L, d),
        pos=rn(N, d) if mode == 1 else None,
        w1=rn(G * m4, d, scale=0.04), b1=rn(G * m4),
        w2=rn(G * d, m4, scale=0.04), b2=rn(G * d),
        gout=rn(B, N, G, d))


@functools.lru_cache(maxsize=None)
def _native(shape, mode, wide, wide8=False):
    """GroupedFFFn forward + backward and the raw forward op; computed once
    per (shape, mode, epilogue mode) and shared by the tests below."""
    from glom_pytorch_amd.ops.functional import GroupedFFFn
    ext = _ext()
    inp = _inputs(shape, mode)
    default = ext.get_wide_epilogue_mode()
    if wide == 2:
        ext.set_wide_epilogue(True)     # the bool binding means "all wide"
        assert ext.get_wide_epilogue_mode() == 2
    elif wide == 0:
        ext.set_wide_epilogue(False)
        assert ext.get_wide_epilogue_mode() == 0
    else:
        ext.set_wide_epilogue_mode(wide)
    ext.set_wide_epilogue_nt8p(wide8)
    try:
        leaves = {k: inp[k].clone().requires_grad_()
                  for k in ("tokens", "levels", "pos", "w1", "b1", "w2", "b2")
                  if inp[k] is not None}
        Y = GroupedFFFn.apply(leaves.get("tokens"), leaves["levels"],
                              leaves.get("pos"), leaves["w1"], leaves["b1"],
                              leaves["w2"], leaves["b2"], mode)
        names = (["tokens", "levels"] if mode == 0 else ["levels", "pos"]) \
            + ["w1", "b1", "w2", "b2"]
        grads = torch.autograd.grad(Y, [leaves[n] for n in names],
                                    inp["gout"])
        Y2, Hpre, Hact, _ = ext.grouped_ff_fwd(
            inp["tokens"], inp["levels"], inp["pos"], inp["w1"], inp["b1"],
            inp["w2"], inp["b2"], mode)
        torch.cuda.synchronize()
    finally:
        ext.set_wide_epilogue_mode(default)
        ext.set_wide_epilogue_nt8p(False)
    out = {"Y": Y.detach(), "Y_op": Y2, "Hpre": Hpre, "Hact": Hact}
    out.update({"d" + n: g for n, g in zip(names, grads)})
    return out


def test_shapes_dispatch_nt5p():
    """Without this the bitwise test could compare nt4 with nt4."""
    code = (
        "import torch\n"
        "from glom_pytorch_amd.ops import _load_extension\n"
        "ext = _load_extension()\n"
        "bf = torch.bfloat16\n"
        "for (B, N, L, d, m4, mode) in %r:\n"
        "    G = L if mode == 0 else L - 1\n"
        "    r = lambda *s: torch.randn(*s, device='cuda:0', dtype=bf)\n"
        "    tok = r(B, N, d) if mode == 0 else None\n"
        "    pos = r(N, d) if mode == 1 else None\n"
        "    lv, w1, w2 = r(B, N, L, d), r(G * m4, d), r(G * d, m4)\n"
        "    Y, hp, ha, tdin = ext.grouped_ff_fwd(tok, lv, pos, w1,\n"
        "        r(G * m4), w2, r(G * d), mode)\n"
        "    ext.grouped_ff_bwd(torch.randn_like(Y), tok, lv, pos, w1, w2,\n"
        "        hp, ha, mode, None, None, tdin)\n"
        "    ext.grouped_ff_fwd(tok, lv, pos, w1, r(G * m4), w2, r(G * d),\n"
        "        mode, False)\n"
        "torch.cuda.synchronize()\n"
        % [SHAPES[s] + (m,) for s, m in CASES + [("C", 0), ("D", 0)]])
    env = dict(os.environ, GLOM_DISPATCH_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", code], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    lines = [ln for ln in r.stderr.splitlines() if "[dispatch]" in ln]
    for s, mode in CASES:
        B, N, L, d, m4 = SHAPES[s]
        key = "L0 M%d N%d K%d " % (B * N, m4, d)
        # EPI_GELU_PAIR = 2 (up), EPI_GELUGRAD = 1 (dH), EPI_GELU = 5
        for epi in (2, 1, 5):
            hit = [ln for ln in lines if key + "epi%d " % epi in ln]
            assert hit, (s, mode, epi, lines)
            assert all("nt5p=1" in ln and "nt8p=0" in ln for ln in hit), hit
    # shape C: the down-projection (N=d, K=m4) belongs to nt8p (the
    # bottom-up dX scatters through a C table and does not)
    B, N, L, d, m4 = SHAPES["C"]
    hit = [ln for ln in lines if "ctabflag=0" in ln
           and "L0 M%d N%d K%d epi0 " % (B * N, d, m4) in ln]
    assert len(hit) >= 2 and all("nt8p=1" in ln for ln in hit), hit
    # shape D: dH with K=2048 -> nt8p's EPI_GELUGRAD epilogue
    B, N, L, d, m4 = SHAPES["D"]
    hit = [ln for ln in lines
           if "L0 M%d N%d K%d epi1 " % (B * N, m4, d) in ln]
    assert hit and all("nt8p=1" in ln for ln in hit), hit


@pytest.mark.parametrize("wide", [1, 2, 3])
@pytest.mark.parametrize("shape,mode", CASES)
def test_wide_epilogue_bitwise_equals_narrow(shape, mode, wide):
    old = _native(shape, mode, 0)
    new = _native(shape, mode, wide)
    assert set(old) == set(new) and len(old) == 10
    for k in old:
        assert old[k].shape == new[k].shape and old[k].numel() > 0, k
        assert torch.equal(old[k], new[k]), k


@pytest.mark.parametrize("shape", ["C", "D"])
def test_nt8p_wide_epilogue_bitwise_equals_narrow(shape):
    old = _native(shape, 0, 2, wide8=False)
    new = _native(shape, 0, 2, wide8=True)
    for k in old:
        assert old[k].numel() > 0 and torch.equal(old[k], new[k]), k


@pytest.mark.parametrize("shape,mode,wide8",
                         [c + (False,) for c in CASES] + [("C", 0, True)])
def test_wide_epilogue_matches_fp32(shape, mode, wide8):
    """Plain randn inputs: every row and column differs, so a wrong
    row/column map in the transposes cannot cancel out."""
    B, N, L, d, m4 = SHAPES[shape]
    G = L if mode == 0 else L - 1
    inp = _inputs(shape, mode)
    new = _native(shape, mode, 2, wide8=wide8)

    f = {k: v.float().requires_grad_() for k, v in inp.items()
         if v is not None and k != "gout"}
    if mode == 0:
        xs = [f["tokens"]] + [f["levels"][..., g, :] for g in range(L - 1)]
    else:
        xs = [f["levels"][..., g + 1, :] + f["pos"] for g in range(G)]
    pre, outs = [], []
    for g in range(G):
        h = xs[g] @ f["w1"][g * m4:(g + 1) * m4].t() \
            + f["b1"][g * m4:(g + 1) * m4]
        pre.append(h)
        outs.append(F.gelu(h) @ f["w2"][g * d:(g + 1) * d].t()
                    + f["b2"][g * d:(g + 1) * d])
    ref = torch.stack(outs, dim=-2)
    names = (["tokens", "levels"] if mode == 0 else ["levels", "pos"]) \
        + ["w1", "b1", "w2", "b2"]
    rgrads = torch.autograd.grad(ref, [f[n] for n in names],
                                 inp["gout"].float())
    hpre = torch.stack([h.detach().reshape(B * N, m4) for h in pre])

    assert _rel(new["Y"], ref) < 1.5e-2
    assert _rel(new["Hpre"], hpre) < 1.5e-2
    assert _rel(new["Hact"], F.gelu(hpre)) < 1.5e-2
    for n, rg in zip(names, rgrads):
        assert _rel(new["d" + n], rg) < 6e-2, (n, _rel(new["d" + n], rg))


@pytest.mark.parametrize("wide", [2, 0])
@pytest.mark.parametrize("shape,mode", CASES)
def test_forward_only_skips_hpre(shape, mode, wide):
    ext = _ext()
    inp = _inputs(shape, mode)
    full = _native(shape, mode, wide)
    default = ext.get_wide_epilogue_mode()
    ext.set_wide_epilogue_mode(wide)
    try:
        Y, Hpre, Hact, _ = ext.grouped_ff_fwd(
            inp["tokens"], inp["levels"], inp["pos"], inp["w1"], inp["b1"],
            inp["w2"], inp["b2"], mode, False)
        torch.cuda.synchronize()
    finally:
        ext.set_wide_epilogue_mode(default)
    assert Hpre.numel() == 0
    assert torch.equal(Y, full["Y_op"])
    assert torch.equal(Hact, full["Hact"])


def _headline_model(seed=0):
    from glom_pytorch_amd import Glom
    torch.manual_seed(seed)
    return Glom(dim=512, levels=6, image_size=224, patch_size=14).to(DEV, BF)


def test_no_grad_forward_unchanged_by_flag():
    """Inference at shape A (B=6): EPI_GELU on every iteration vs the
    pre-activation kept everywhere, as before the flag existed."""
    from glom_pytorch_amd.ops import functional as fn
    m = _headline_model()
    img = torch.randn(6, 3, 224, 224, device=DEV).to(BF)
    assert fn.FORCE_SAVE_FOR_BWD is False
    with torch.no_grad():
        a = m(img, iters=3, return_all=True)
        fn.FORCE_SAVE_FOR_BWD = True
        try:
            b = m(img, iters=3, return_all=True)
        finally:
            fn.FORCE_SAVE_FOR_BWD = False
    assert torch.equal(a, b)


def test_training_step_unchanged_by_flag():
    """One DenoisingTrainer step with the forward-only tail overlapped
    (decode at t=2 of 3 iterations -> one tail iteration)."""
    from glom_pytorch_amd.ops import functional as fn
    from glom_pytorch_amd.parallel.trainer import DenoisingTrainer

    def trainer():
        return DenoisingTrainer(_headline_model(), lr=1e-3, noise_std=0.0,
                                decode_step=2, graph_step=False,
                                overlap_tail=True)
    img = torch.randn(6, 3, 224, 224, device=DEV).to(BF)
    ta, tb = trainer(), trainer()
    tb.model.load_state_dict(ta.model.state_dict())
    tb.decoder.load_state_dict(ta.decoder.state_dict())
    with torch.no_grad():
        for mw, q in zip(tb.master, tb._params):
            mw.copy_(q.float())
    la = ta.step(img, iters=3)
    fn.FORCE_SAVE_FOR_BWD = True
    try:
        lb = tb.step(img, iters=3)
    finally:
        fn.FORCE_SAVE_FOR_BWD = False
    assert la == lb, (la, lb)
    for (na, pa), (_, pb) in zip(ta.model.named_parameters(),
                                 tb.model.named_parameters()):
        assert torch.equal(pa, pb), na


@pytest.mark.parametrize("C", [2048, 1001])   # 16-byte path / scalar path
def test_colsum_fixed_order(C):
    """ext.colsum = k_colsum_part + k_colsum_fin. M=1536 -> 24 row chunks
    of 64: k_colsum_fin runs one unrolled batch of 16 and an 8-row tail.
    The host loop below adds the same f32 values in the same order."""
    M, RB, chunk = 1536, 24, 64
    x = torch.randn(M, C, device=DEV, generator=torch.Generator(
        device=DEV).manual_seed(C)).to(BF)
    out = _ext().colsum(x)
    xv = x.float().view(RB, chunk, C)
    part = torch.zeros(RB, C, device=DEV)
    for r in range(chunk):
        part = part + xv[:, r]
    tot = torch.zeros(C, device=DEV)
    for rc in range(RB):
        tot = tot + part[rc]
    assert torch.equal(out, tot.to(BF))
    # and against the plain reduction: one bf16 ulp (2^-8 relative) of
    # output rounding plus f32 reordering noise (<< 1e-2 at |sum| ~ 40)
    ref = x.float().sum(0)
    assert ((out.float() - ref).abs() <= ref.abs() * 2.0 ** -8 + 1e-2).all()
