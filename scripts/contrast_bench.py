"""Column-contrastive loss, native HIP path against the module's own torch
implementation on the same bf16 GPU tensors: forward and forward+backward
at B*N = 16384, D = 512 (the headline batch) and at B = 16. Device-event
timing, warm-up, interleaved repeats; reports the median and spread, the
native path's achieved TFLOP/s (forward 2*M^2*D, backward 4x that: two
logit recomputes and two G' products), the peak memory of one
forward+backward, and the fast-tile kernel against the generic kernel as
host of the epilogues. Writes the table to --out.

    python scripts/contrast_bench.py [--out FILE] [--reps 10] [--torch-reps 3]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from glom_pytorch_amd import contrast
from glom_pytorch_amd.ops import _load_extension

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/contrast_bench.txt")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--torch-reps", type=int, default=3)
ap.add_argument("--batches", type=int, nargs="+", default=[64, 16])
ap.add_argument("--patches", type=int, default=256)
ap.add_argument("--dim", type=int, default=512)
ap.add_argument("--temperature", type=float, default=0.1)
args = ap.parse_args()

assert torch.cuda.is_available(), "contrast_bench needs a GPU"
ext = _load_extension()      # fail here, not mid-run, if it is not built
dev = "cuda"
N, D, T = args.patches, args.dim, args.temperature
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def inputs(B):
    """Shared direction + per-image direction + noise, second view = first
    + noise: both negative modes are non-degenerate."""
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    a = r(1, 1, D) + 0.6 * r(B, 1, D) + 0.6 * r(B, N, D)
    b = a + 0.6 * r(B, N, D)
    return a.bfloat16(), b.bfloat16()


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def bench(variants, reps, warmup=3):
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            out[name].append(timed(fn))
    return out


def row(name, ms, flops=None):
    med = statistics.median(ms)
    s = (f"{name:<40s} median {med:9.3f} ms   min {min(ms):9.3f}   "
         f"max {max(ms):9.3f}   n={len(ms)}")
    if flops:
        s += f"   {flops / (med * 1e-3) / 1e12:7.1f} TF"
    say(s)
    return med


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


say(f"# contrast_bench: N={N} D={D} temperature={T} negatives=other_images, "
    f"bf16 inputs")
say(f"# device: {torch.cuda.get_device_name(0)}; device events; "
    f"TF = model FLOPs / median time")
ok = True
for B in args.batches:
    M = B * N
    a, b = inputs(B)
    ag = a.clone().requires_grad_(True)
    bg = b.clone().requires_grad_(True)
    fwd_flops = 2.0 * M * M * D

    def n_fwd():
        with torch.no_grad():
            return contrast.column_contrastive_loss(a, b, T)

    def n_both():
        ag.grad = bg.grad = None
        contrast.column_contrastive_loss(ag, bg, T).backward()

    def t_fwd():
        with torch.no_grad():
            return contrast._torch_loss(a, b, T, "other_images")

    def t_both():
        ag.grad = bg.grad = None
        contrast._torch_loss(ag, bg, T, "other_images").backward()

    say()
    say(f"## B={B}: M={M} rows, logits {M}x{M} "
        f"({M * M * 4 / 2 ** 30:.2f} GiB in fp32)")
    before = contrast.native_calls()
    res = bench([("native forward", n_fwd),
                 ("native forward+backward", n_both)], args.reps)
    assert contrast.native_calls() > before
    nf = row("native forward", res["native forward"], fwd_flops)
    nb = row("native forward+backward", res["native forward+backward"],
             5 * fwd_flops)
    say(f"{'native backward (difference of medians)':<40s} "
        f"{nb - nf:16.3f} ms   "
        f"{4 * fwd_flops / ((nb - nf) * 1e-3) / 1e12:7.1f} TF")
    say(f"native peak memory, forward+backward: {peak_mib(n_both):9.1f} MiB")

    # the generic kernel as host of the same epilogues
    ext.set_nce_fast(False)
    try:
        g = bench([("generic-kernel forward", n_fwd),
                   ("generic-kernel forward+backward", n_both)], args.reps)
    finally:
        ext.set_nce_fast(True)
    gf = row("generic-kernel forward", g["generic-kernel forward"], fwd_flops)
    gb = row("generic-kernel forward+backward",
             g["generic-kernel forward+backward"], 5 * fwd_flops)
    say(f"fast-tile host against generic host: forward {gf / nf:.2f}x, "
        f"forward+backward {gb / nb:.2f}x")

    try:
        tres = bench([("torch forward", t_fwd),
                      ("torch forward+backward", t_both)], args.torch_reps,
                     warmup=1)
        tf = row("torch forward", tres["torch forward"])
        tb = row("torch forward+backward", tres["torch forward+backward"])
        say(f"torch peak memory, forward+backward:  {peak_mib(t_both):9.1f} "
            f"MiB")
        say(f"speedup: forward {tf / nf:.1f}x, forward+backward "
            f"{tb / nb:.1f}x")
        with torch.no_grad():
            d = abs(n_fwd().item() - t_fwd().item())
        say(f"check: |native - torch| loss {d:.2e}")
        ok = ok and nb < tb and d < 1e-3
    except torch.cuda.OutOfMemoryError:
        say("torch path: out of memory at this size")
    del a, b, ag, bg
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
say(f"wrote {args.out}")
assert ok, "native path slower than torch, or results differ"
