"""Within-process interleaved A/B of the TN weight-gradient GEMMs: the
repack kernels (gemm_tn_sk / gemm_tn_fast) vs the direct-to-LDS +
transposed-read kernel (gemm_tn_tr, split-K pipeline variants 1..3), and
the scalar vs re-blocked split-K finish. bench_gemm times the GEMM and,
where the call is split, its finish together. Rounds alternate the variants
in ONE process; operands are random. As a ceiling, the NT layout at the same
(M, N, K, G) is printed (no split-K, no finish).

    python scripts/tn_tr_ab.py
"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from glom_pytorch_amd.ops import _load_extension
ext = _load_extension()
torch.manual_seed(0)

ROUNDS = 10
LAYOUT_NT, LAYOUT_TN = 0, 2


def fmt(xs):
    xs = sorted(xs)
    return f"{xs[len(xs) // 2]:6.1f} [{xs[0]:6.1f}, {xs[-1]:6.1f}]"


def setup(tr, variant, finw):
    def f():
        ext.set_tn_tr(tr)
        ext.set_tn_tr_variant(variant)
        ext.set_finish_wide(finw)
    return f


SPLIT = [("old", setup(False, 1, False)),
         ("old + finish4", setup(False, 1, True)),
         ("tr BK64x2", setup(True, 1, True)),
         ("tr BK32x3", setup(True, 2, True)),
         ("tr BK32x2", setup(True, 3, True))]
NOSPLIT = [("old", setup(False, 1, True)), ("tr BK64x2", setup(True, 1, True))]


def ab(name, M, N, K, G, reps, variants):
    fl = 2.0 * M * N * K * G
    res = {lab: [] for lab, _ in variants}
    for _ in range(ROUNDS):
        for lab, st in variants:
            st()
            ms = ext.bench_gemm(M, N, K, LAYOUT_TN, G, 0, reps)
            res[lab].append(fl / (ms / 1e3) / 1e12)
    nt = [fl / (ext.bench_gemm(M, N, K, LAYOUT_NT, G, 0, reps) / 1e3) / 1e12
          for _ in range(3)]
    print(f"{name:20s} M{M} N{N} K{K} G{G}  TF median [min, max]")
    for lab, _ in variants:
        print(f"    {lab:14s} {fmt(res[lab])}")
    print(f"    {'NT ceiling':14s} {fmt(nt)}")
    sys.stdout.flush()


mode, var = ext.get_tn_tr_mode(), ext.get_tn_tr_variant()
try:
    ab("dW1 headline", 2048, 512, 16384, 6, 20, SPLIT)
    ab("dW2 headline", 512, 2048, 16384, 6, 20, SPLIT)
    ab("dW1 headline td", 2048, 512, 16384, 5, 20, SPLIT)
    ab("dW2 headline td", 512, 2048, 16384, 5, 20, SPLIT)
    ab("dW1 stretch", 4096, 1024, 8192, 12, 8, NOSPLIT)
    ab("dW2 stretch", 1024, 4096, 8192, 12, 8, NOSPLIT)
    ab("non-split K=4096", 1024, 1024, 4096, 64, 8, NOSPLIT)
    ab("non-split K=1024", 1024, 1024, 1024, 64, 20, NOSPLIT)
    ab("attention dv/dk", 256, 512, 256, 384, 20, NOSPLIT)
finally:
    ext.set_tn_tr_mode(mode)
    ext.set_tn_tr_variant(var)
    ext.set_finish_wide(True)
