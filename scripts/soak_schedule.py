"""Does a warmup + cosine schedule (and no weight decay on biases and
embeddings) buy bf16 training stability at the headline config, and what
does the device-resident schedule cost per step?

    python scripts/soak_schedule.py soak          # 8 runs, one JSON line each
    python scripts/soak_schedule.py cost none     # step time, no schedule (graphed)
    python scripts/soak_schedule.py cost cosine   # ... with a cosine schedule (eager launches)

soak: headline model, B=16, noise_std=0.3, 150 steps of the
scripts/soak_matrix.py structured images, native bf16; lr in {3e-4, 1e-3},
constant against 40 warmup steps + cosine to step 150, with and without
no_decay.

cost: 20 steps after 5 warmup steps at the headline config (B=64), three
repeats, host clock around work that ends in a device synchronise. Without
a schedule the trainer replays its captured step; with one it launches
eagerly, and the JSON line says which ("graphed").
``cost none`` uses nothing this feature added, so it also runs against an
older checkout of the package: point GLOM_PKG_ROOT at that checkout's root.
Results are recorded in profiles/README.md."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.environ.get(
    "GLOM_PKG_ROOT",
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from glom_pytorch_amd import Glom
from glom_pytorch_amd.parallel.trainer import DenoisingTrainer

HEADLINE = dict(dim=512, levels=6, image_size=224, patch_size=14)


def structured_batch(B, dev, dtype, size=224):
    """The scripts/soak_matrix.py images: sums of four random sinusoids."""
    y, x = torch.meshgrid(torch.linspace(0, 1, size, device=dev),
                          torch.linspace(0, 1, size, device=dev),
                          indexing="ij")
    img = torch.zeros(B, 3, size, size, device=dev)
    for _ in range(4):
        fx, fy = torch.randint(1, 5, (2,), device=dev)
        ph = torch.rand(B, 3, 1, 1, device=dev) * 2 * math.pi
        amp = torch.randn(B, 3, 1, 1, device=dev) * 0.5
        img += amp * torch.sin(2 * math.pi * (fx * x + fy * y) + ph)
    return img.to(dtype)


def soak(steps):
    from glom_pytorch_amd.ops.optim import LRSchedule
    for lr in (3e-4, 1e-3):
        for sched in (None, "cosine"):
            for no_decay in (False, True):
                torch.manual_seed(0)
                model = Glom(**HEADLINE).to("cuda", torch.bfloat16)
                schedule = (LRSchedule("cosine", warmup_steps=40,
                                       total_steps=steps)
                            if sched else None)
                tr = DenoisingTrainer(model, lr=lr, noise_std=0.3,
                                      lr_schedule=schedule,
                                      no_decay=no_decay)
                losses = [tr.step(structured_batch(16, "cuda",
                                                   torch.bfloat16), iters=12)
                          for _ in range(steps)]
                print(json.dumps({
                    "lr": lr, "schedule": sched or "constant",
                    "no_decay": no_decay,
                    "first10": sum(losses[:10]) / 10,
                    "l50": losses[49], "l100": losses[99],
                    "last10": sum(losses[-10:]) / 10,
                    "max": max(losses),
                    "final_lr": tr.current_lr()}), flush=True)


def cost(variant, steps, warmup, repeats):
    kw = {}
    if variant == "cosine":
        from glom_pytorch_amd.ops.optim import LRSchedule
        kw["lr_schedule"] = LRSchedule(
            "cosine", warmup_steps=10, total_steps=warmup + steps * repeats)
    torch.manual_seed(0)
    model = Glom(**HEADLINE).to("cuda", torch.bfloat16)
    tr = DenoisingTrainer(model, lr=1e-4, noise_std=0.3, **kw)
    img = torch.randn(64, 3, 224, 224, device="cuda", dtype=torch.bfloat16)
    for _ in range(warmup):
        tr.step(img, iters=12, sync_loss=False)
    torch.cuda.synchronize()
    graphed = bool(tr._graphs) and all(tr._graphs.values())
    assert graphed == (variant == "none"), "unexpected launch mode"
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = tr.step(img, iters=12, sync_loss=False)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    print(json.dumps({"variant": variant, "graphed": graphed,
                      "package": os.path.dirname(
                          sys.modules["glom_pytorch_amd"].__file__),
                      "ms_per_step": [round(m, 3) for m in ms],
                      "loss": float(loss)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("soak")
    s.add_argument("--steps", type=int, default=150)
    c = sub.add_parser("cost")
    c.add_argument("variant", choices=["none", "cosine"])
    c.add_argument("--steps", type=int, default=20)
    c.add_argument("--warmup", type=int, default=5)
    c.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: no fallback"
    if a.cmd == "soak":
        soak(a.steps)
    else:
        cost(a.variant, a.steps, a.warmup, a.repeats)
