"""bench.py command line: --dump-outputs writes what the last timed step
computed, --full is accepted, and the result line keeps its fields."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench  # repo root is on sys.path (conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_large_tensors_reproducibly(tmp_path):
    big = torch.arange(bench.DUMP_MAX_ELEMS + 1000, dtype=torch.float32)
    small = torch.randn(3, 5).to(torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("big", big), ("small", small)])
    a_big = np.load(tmp_path / "a" / "big.npy")
    assert a_big.dtype == np.float32
    assert a_big.shape == (bench.DUMP_MAX_ELEMS,)
    # values are their own positions: a sample, not a prefix, same each time
    assert a_big.max() >= bench.DUMP_MAX_ELEMS
    assert np.array_equal(a_big, np.load(tmp_path / "b" / "big.npy"))
    a_small = np.load(tmp_path / "a" / "small.npy")
    assert a_small.dtype == np.float32 and a_small.shape == (3, 5)
    assert np.array_equal(a_small, small.float().numpy())


def test_dump_outputs_budget_with_many_midsize_tensors(tmp_path):
    # 40 tensors just under the per-tensor cap would be 160 MB if written
    # whole: the cap shrinks to an equal share of the 64 MB budget
    t = torch.zeros(bench.DUMP_MAX_ELEMS - 1).expand(40, -1)
    bench.dump_outputs(str(tmp_path), [(f"t{i}", t[i]) for i in range(40)])
    sizes = [np.load(tmp_path / f"t{i}.npy").nbytes for i in range(40)]
    assert sum(sizes) <= bench.DUMP_MAX_BYTES
    assert min(sizes) == max(sizes) > bench.DUMP_MAX_BYTES // 40 - 8


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")
def test_bench_full_run_dumps_last_step(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", "--batch", "2", "--dim", "64",
         "--levels", "3", "--image-size", "32", "--patch-size", "8",
         "--iters", "3", "--full", "--dump-outputs", str(out)],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["metric"] == "images/sec" and res["unit"] == "images/sec"
    assert res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["steps"] == 3
    assert res["value"] == pytest.approx(2 * 1e3 / res["ms_per_step"])

    files = sorted(os.listdir(out))
    assert "loss.npy" in files
    assert "model.bottom_up.net.1.weight.npy" in files
    assert "master.model.bottom_up.net.1.weight.npy" in files
    total = 0
    for f in files:
        arr = np.load(out / f)
        assert arr.dtype == np.float32, f
        assert np.isfinite(arr).all(), f
        total += arr.nbytes
    assert total <= 64 * 10 ** 6
    assert float(np.load(out / "loss.npy")) == pytest.approx(res["loss_last"])
