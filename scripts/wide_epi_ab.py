"""Within-process interleaved A/B of the register epilogues: 2-byte
fragment-order accesses vs the 16-byte transposed ones
(set_wide_epilogue_mode: 0 narrow, 2 all wide, 3 wide aux loads only;
set_wide_epilogue_nt8p), on the GEMM shapes of the headline step. Rounds
alternate the two variants in ONE process; operands are random.

    python scripts/wide_epi_ab.py            # nt5p shapes + nt8p down-proj
    GLOM_NT8P_MINK=512 python scripts/wide_epi_ab.py --nt8p-k512
        # K=512 dH on nt8p (narrow / wide) vs nt5p wide
"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from glom_pytorch_amd.ops import _load_extension
ext = _load_extension()
torch.manual_seed(0)

ROUNDS = 10
EPI_NONE, EPI_GELUGRAD, EPI_GELU_PAIR, EPI_GELU = 0, 1, 2, 5


def fmt(xs):
    xs = sorted(xs)
    return f"{xs[len(xs) // 2]:6.1f} [{xs[0]:6.1f}, {xs[-1]:6.1f}]"


def ab(name, M, N, K, G, epi, reps, variants):
    """variants: list of (label, setup callable); interleaved per round."""
    fl = 2.0 * M * N * K * G
    res = {lab: [] for lab, _ in variants}
    for _ in range(ROUNDS):
        for lab, setup in variants:
            setup()
            ms = ext.bench_gemm(M, N, K, 0, G, epi, reps)
            res[lab].append(fl / (ms / 1e3) / 1e12)
    print(f"{name:22s} M{M} N{N} K{K} G{G} epi{epi}  TF median [min, max]")
    for lab, _ in variants:
        print(f"    {lab:14s} {fmt(res[lab])}")
    sys.stdout.flush()


def nt5p(mode):
    def f():
        ext.set_nt8p(True)
        ext.set_wide_epilogue_mode(mode)
    return f


def nt8p(wide):
    def f():
        ext.set_nt8p(True)
        ext.set_wide_epilogue_nt8p(wide)
    return f


def nt5p_only():
    ext.set_nt8p(False)
    ext.set_wide_epilogue_mode(2)


if "--nt8p-k512" in sys.argv:
    assert os.environ.get("GLOM_NT8P_MINK") == "512", "set GLOM_NT8P_MINK=512"
    ab("dH K=512", 16384, 2048, 512, 5, EPI_GELUGRAD, 30,
       [("nt5p wide", nt5p_only), ("nt8p narrow", nt8p(False)),
        ("nt8p wide", nt8p(True))])
else:
    two = [("narrow", nt5p(0)), ("wide", nt5p(2))]
    ab("up-proj GELU_PAIR", 16384, 2048, 512, 6, EPI_GELU_PAIR, 30, two)
    ab("up-proj GELU (no Hpre)", 16384, 2048, 512, 6, EPI_GELU, 30, two)
    ab("up-proj plain", 16384, 2048, 512, 6, EPI_NONE, 30, two)
    ab("dH GELUGRAD", 16384, 2048, 512, 5, EPI_GELUGRAD, 30,
       two + [("wide aux only", nt5p(3))])
    ab("down-proj (nt8p)", 16384, 512, 2048, 6, EPI_NONE, 30,
       [("narrow", nt8p(False)), ("wide", nt8p(True))])
    ab("square 2048 (nt8p)", 16384, 2048, 2048, 6, EPI_NONE, 15,
       [("narrow", nt8p(False)), ("wide", nt8p(True))])
