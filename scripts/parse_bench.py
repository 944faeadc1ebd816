"""Parse trees on the headline trajectory slab (13,64,256,6,512) bf16:
native HIP kernels vs the module's own torch implementation on the same
GPU tensors. Device-event timing, warm-up, interleaved repeats; reports
median and spread, and for island_means the achieved GB/s as (bytes read +
bytes written) / time. Writes the table to --out (default
profiles/parse_bench.txt).

    python scripts/parse_bench.py [--out FILE] [--reps 10] [--torch-reps 3]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from glom_pytorch_amd import islands, parse
from glom_pytorch_amd.ops import _load_extension

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/parse_bench.txt")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--torch-reps", type=int, default=3)
ap.add_argument("--shape", type=int, nargs=5, default=[13, 64, 256, 6, 512],
                metavar=("T1", "B", "N", "L", "D"))
ap.add_argument("--threshold", type=float, default=0.9)
args = ap.parse_args()

assert torch.cuda.is_available(), "parse_bench needs a GPU"
_load_extension()            # fail here, not mid-run, if it is not built
dev = "cuda"
T1, B, N, L, D = args.shape
side = int(N ** 0.5)
assert side * side == N
thr = args.threshold
grid = (side, side)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


# structured slab as in islands_bench.py: level l is made of (s x s)-cell
# blocks that share a random prototype, plus noise (within-block cosine
# ~0.96, across ~0), so there are real islands, nested across levels
torch.manual_seed(0)
slab = torch.empty(T1, B, N, L, D, device=dev, dtype=torch.bfloat16)
for l in range(L):
    s = min(side, (1, 2, 2, 4, 4, 8)[l % 6])
    proto = torch.randn(T1, B, side // s, side // s, D, device=dev)
    proto = proto.repeat_interleave(s, 2).repeat_interleave(s, 3)
    lvl = proto + 0.2 * torch.randn(T1, B, side, side, D, device=dev)
    slab[:, :, :, l] = lvl.reshape(T1, B, N, D).to(torch.bfloat16)
    del proto, lvl
labels = islands.island_labels(slab, thr, grid)
slab_bytes = slab.numel() * 2
label_bytes = labels.numel() * 4
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


def moved(out_elem_bytes):
    """Bytes island_means has to read and write: slab + labels in, every
    output row out."""
    return slab_bytes + label_bytes + slab.numel() * out_elem_bytes


cnt = islands.island_count(labels).float().mean(dim=(0, 1)).tolist()
say(f"# parse_bench: slab {(T1, B, N, L, D)} bf16 = "
    f"{slab_bytes / 1e9:.3f} GB, grid {side}x{side}, threshold {thr}, "
    f"mean islands per level {[round(v, 1) for v in cnt]}")
say(f"# device: {torch.cuda.get_device_name(0)}; device events; "
    f"GB/s = (slab + labels read + output written) / median time")

BF, F32 = torch.bfloat16, torch.float32
native = [
    ("native island_parents",
     lambda: parse.island_parents(labels, return_overlap=True), None),
    ("native island_means f32 root",
     lambda: parse.island_means(slab, labels), moved(4)),
    ("native island_means f32 broadcast",
     lambda: parse.island_means(slab, labels, True), moved(4)),
    ("native island_means bf16 root",
     lambda: parse.island_means(slab, labels, False, BF), moved(2)),
    ("native island_means bf16 broadcast",
     lambda: parse.island_means(slab, labels, True, BF), moved(2)),
    ("native parse_tree (labels..means)",
     lambda: parse.parse_tree(slab, thr, grid), None),
]
res = bench([(n, f) for n, f, _ in native], args.reps)
med = {}
for name, _, b in native:
    med[name] = row(name, res[name], b)

say()


def torch_tree():
    agr = islands._torch_agreement(slab, side, side, 2)
    lab = islands._torch_labels(agr, thr)
    islands._torch_sizes(lab)
    parse._torch_parents(lab)
    parse._torch_means(slab, lab, False, F32)


tor = [
    ("torch island_parents",
     lambda: parse._torch_parents(labels), None),
    ("torch island_means f32 root",
     lambda: parse._torch_means(slab, labels, False, F32), moved(4)),
    ("torch island_means bf16 broadcast",
     lambda: parse._torch_means(slab, labels, True, BF), moved(2)),
    ("torch parse_tree (labels..means)", torch_tree, None),
]
with torch.no_grad():
    rest = bench([(n, f) for n, f, _ in tor], args.torch_reps, warmup=1)
for name, _, b in tor:
    med[name] = row(name, rest[name], b)

say()
for what in ("island_parents", "island_means f32 root",
             "island_means bf16 broadcast",
             "parse_tree (labels..means)"):
    n, t = med[f"native {what}"], med[f"torch {what}"]
    say(f"speedup {what}: {t / n:7.1f}x  "
        f"(torch {t:.3f} ms / native {n:.3f} ms)")

# the two paths must agree at this size too: parents and overlap exactly,
# means within the fp32 summation bound (N+1) * 2**-24 * max|levels|
par, ovl = parse.island_parents(labels, return_overlap=True)
with torch.no_grad():
    tpar, tovl = parse._torch_parents(labels)
same = bool(torch.equal(par, tpar) and torch.equal(ovl, tovl))
say(f"check: native parents/overlap == torch: {same}")
ok = same
bound = (N + 1) * 2.0 ** -24 * slab.float().abs().max().item()
for bc in (False, True):
    a = parse.island_means(slab, labels, bc)
    b = parse.island_means(slab, labels, bc)
    rep = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    del b
    with torch.no_grad():
        t = parse._torch_means(slab, labels, bc, F32)
    err = (a - t).abs().max().item()
    del a, t
    say(f"check broadcast={bc}: max |native - torch| means {err:.2e} "
        f"(bound 2 x {bound:.2e}); native bitwise repeatable: {rep}")
    ok = ok and rep and err <= 2 * bound

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
say(f"wrote {args.out}")
assert ok, "native and torch results differ"
