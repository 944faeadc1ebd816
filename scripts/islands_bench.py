"""Island analysis on the headline trajectory slab (13,64,256,6,512) bf16:
native HIP kernels vs the module's own torch implementation on the same
GPU tensor. Device-event timing, warm-up, interleaved repeats; reports
median and spread, and the agreement kernel's achieved GB/s (slab bytes /
time). Writes the table to --out (default profiles/islands_bench.txt).

    python scripts/islands_bench.py [--out FILE] [--reps 10] [--torch-reps 3]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from glom_pytorch_amd import islands
from glom_pytorch_amd.ops import _load_extension

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/islands_bench.txt")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--torch-reps", type=int, default=3)
ap.add_argument("--shape", type=int, nargs=5, default=[13, 64, 256, 6, 512],
                metavar=("T1", "B", "N", "L", "D"))
ap.add_argument("--threshold", type=float, default=0.9)
args = ap.parse_args()

assert torch.cuda.is_available(), "islands_bench needs a GPU"
_load_extension()            # fail here, not mid-run, if it is not built
dev = "cuda"
T1, B, N, L, D = args.shape
side = int(N ** 0.5)
assert side * side == N
thr = args.threshold
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


# structured slab: level l is made of (s x s)-cell blocks that share a
# random prototype, plus noise (within-block cosine ~0.96, across ~0), so
# the labelling has real islands to find at threshold 0.9
torch.manual_seed(0)
slab = torch.empty(T1, B, N, L, D, device=dev, dtype=torch.bfloat16)
for l in range(L):
    s = min(side, (1, 2, 2, 4, 4, 8)[l % 6])
    proto = torch.randn(T1, B, side // s, side // s, D, device=dev)
    proto = proto.repeat_interleave(s, 2).repeat_interleave(s, 3)
    lvl = proto + 0.2 * torch.randn(T1, B, side, side, D, device=dev)
    slab[:, :, :, l] = lvl.reshape(T1, B, N, D).to(torch.bfloat16)
    del proto, lvl
slab_bytes = slab.numel() * 2
torch.cuda.synchronize()


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def bench(variants, reps, warmup=3):
    """Interleaved rounds over the variants; {name: [ms, ...]}."""
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            out[name].append(timed(fn))
    return out


def row(name, ms, bytes_=None):
    med = statistics.median(ms)
    s = (f"{name:<44s} median {med:9.3f} ms   min {min(ms):9.3f}   "
         f"max {max(ms):9.3f}   n={len(ms)}")
    if bytes_:
        s += f"   {bytes_ / (med * 1e-3) / 1e9:8.1f} GB/s"
    say(s)
    return med


say(f"# islands_bench: slab {(T1, B, N, L, D)} bf16 = "
    f"{slab_bytes / 1e9:.3f} GB, grid {side}x{side}, threshold {thr}")
say(f"# device: {torch.cuda.get_device_name(0)}; device events; "
    f"GB/s = slab bytes / median time")

grid = (side, side)
native = []
for conn in (4, 8):
    native.append((f"native edge_agreement c{conn}",
                   lambda c=conn: islands.edge_agreement(slab, grid, c)))
    native.append((f"native island_labels c{conn} (agreement+labels)",
                   lambda c=conn: islands.island_labels(slab, thr, grid, c)))
res = bench(native, args.reps)
med = {}
for name, _ in native:
    med[name] = row(name, res[name],
                    slab_bytes if "edge_agreement" in name else None)

# labelling kernel alone, on a fixed agreement tensor
for conn in (4, 8):
    agr = islands.edge_agreement(slab, grid, conn)
    r = bench([(f"native labels_from_agreement c{conn}",
                lambda: islands.labels_from_agreement(agr, thr, conn))],
              args.reps)
    for k, v in r.items():
        row(k, v)
    del agr

say()
C = {4: 2, 8: 4}
tor = []
for conn in (4, 8):
    tor.append((f"torch edge_agreement c{conn}",
                lambda c=conn: islands._torch_agreement(slab, side, side,
                                                        C[c])))
    tor.append((f"torch island_labels c{conn} (agreement+labels)",
                lambda c=conn: islands._torch_labels(
                    islands._torch_agreement(slab, side, side, C[c]), thr)))
with torch.no_grad():
    rest = bench(tor, args.torch_reps, warmup=1)
for name, _ in tor:
    med[name] = row(name, rest[name],
                    slab_bytes if "edge_agreement" in name else None)

say()
ok = True
for conn in (4, 8):
    for what in ("edge_agreement", "island_labels"):
        tail = "" if what == "edge_agreement" else " (agreement+labels)"
        n = med[f"native {what} c{conn}{tail}"]
        t = med[f"torch {what} c{conn}{tail}"]
        say(f"speedup {what} c{conn}: {t / n:7.1f}x  "
            f"(torch {t:.3f} ms / native {n:.3f} ms)")
        ok = ok and n < t

# the two paths must agree at this size too: labels are exact given the
# agreement they were decided on
for conn in (4, 8):
    lab, agr = islands.island_labels(slab, thr, grid, conn,
                                     return_agreement=True)
    with torch.no_grad():
        want = islands._torch_labels(agr, thr)
        tagr = islands._torch_agreement(slab, side, side, C[conn])
    same = bool(torch.equal(lab, want))
    derr = (agr - tagr).abs().max().item()
    cnt = islands.island_count(lab).float().mean(dim=(0, 1)).tolist()
    say(f"check c{conn}: native labels == torch labels of the same "
        f"agreement: {same}; max |native - torch| agreement {derr:.2e}; "
        f"mean islands per level {[round(v, 1) for v in cnt]}")
    ok = ok and same

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
say(f"wrote {args.out}")
assert ok, "native path slower than torch, or results differ"
