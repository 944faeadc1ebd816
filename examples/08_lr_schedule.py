"""Warmup + cosine learning-rate schedule with no weight decay on biases and
embeddings, and a resumed run that continues the curve where the saved one
stopped.

On the native bf16 GPU path the schedule is evaluated on the device from the
fused optimizer's step counter (such a trainer launches its steps eagerly;
the captured step keeps lr as a kernel argument). On CPU (here, when no GPU is present) the trainer sets torch.optim.AdamW's
group lr from the same formula."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from glom_pytorch_amd import Glom
from glom_pytorch_amd.ops.optim import LRSchedule
from glom_pytorch_amd.parallel.trainer import DenoisingTrainer

use_gpu = torch.cuda.is_available()
dev = "cuda" if use_gpu else "cpu"
dtype = torch.bfloat16 if use_gpu else torch.float32
cfg = dict(dim=64, levels=3, image_size=32, patch_size=8)
steps, save_at = 12, 6
schedule = LRSchedule("cosine", warmup_steps=3, total_steps=steps,
                      min_ratio=0.1)


def make_trainer(lr_schedule):
    torch.manual_seed(0)
    model = Glom(**cfg).to(dev, dtype)
    return DenoisingTrainer(model, lr=1e-3, noise_std=0.3,
                            lr_schedule=lr_schedule, no_decay=True)


torch.manual_seed(1)
batches = [torch.randn(2, 3, 32, 32, device=dev, dtype=dtype)
           for _ in range(steps)]

with tempfile.TemporaryDirectory() as ckpt_dir:
    path = os.path.join(ckpt_dir, "sched_ckpt.pt")
    trainer = make_trainer(schedule)
    curve = []
    for k, img in enumerate(batches):
        loss = trainer.step(img, iters=6)
        curve.append(trainer.current_lr())
        print(f"step {k:2d}: lr {curve[-1]:.3e} "
              f"(factor {schedule.factor(k):.3f})  loss {loss:.4f}")
        if k + 1 == save_at:
            trainer.save_checkpoint(path)

    # the checkpoint carries the schedule, the base lr and the step count
    resumed = make_trainer(None)
    resumed.load_checkpoint(path)
    print(f"resumed at step {resumed.step_idx} with {resumed.lr_schedule}")
    for k in range(save_at, steps):
        resumed.step(batches[k], iters=6)
        lr = resumed.current_lr()
        print(f"step {k:2d}: lr {lr:.3e} (resumed)")
        assert abs(lr - curve[k]) <= 1e-6 * 1e-3, (k, lr, curve[k])
print("resumed run continued the schedule")
