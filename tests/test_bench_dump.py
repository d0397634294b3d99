"""bench.py --dump-outputs on the CPU rehearsal (one process, no GPU): the file holds the timed step's
output, and two runs with the same arguments write the same bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--batch-per-gpu", "3", "--device", "cpu", "--dump-outputs", str(out_dir), *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(env, OMP_NUM_THREADS="2"), cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "output.npy"))


def test_dump_outputs_cpu_is_the_step_output_and_repeats(tmp_path):
    rec, y = _run(tmp_path / "a")
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and rec["vs_baseline"] is None
    assert abs(rec["value"] - 3 * 1e3 / rec["ms_per_step"]) <= 1e-3 * rec["value"]
    assert rec["dumped_outputs"]["output"] == {"shape": [3, 13, 13, 256], "written": [3, 13, 13, 256], "dtype": "float32"}
    assert y.dtype == np.float32 and y.shape == (3, 13, 13, 256)
    _, y2 = _run(tmp_path / "b")
    assert np.array_equal(y, y2)
    # the same seeded input through the CPU engine in this process
    sys.path.insert(0, ROOT)
    from anx.models.alexnet_blocks import AlexNetBlocks
    x = torch.rand((3, 227, 227, 3), generator=torch.Generator().manual_seed(1234)) * 0.1
    ref = AlexNetBlocks(init="rand", seed=1234, device="cpu")(x)
    torch.testing.assert_close(torch.from_numpy(y), ref, rtol=0, atol=0)


def test_dump_outputs_samples_above_the_size_limit(tmp_path, monkeypatch):
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "8")  # importing bench sets it: undone when this test ends
    monkeypatch.syspath_prepend(ROOT)
    import bench
    big = torch.arange(bench.DUMP_BYTES // 4 + 1000, dtype=torch.float32).view(-1, 8)
    small = torch.ones(5, dtype=torch.float64)
    d = bench.dump_outputs(str(tmp_path), {"big": big, "small": small})
    a, s = np.load(tmp_path / "big.npy"), np.load(tmp_path / "small.npy")
    assert s.dtype == np.float64 and s.shape == (5,) and d["big"]["shape"] == list(big.shape)
    assert a.dtype == np.float32 and a.ndim == 1 and a.nbytes <= bench.DUMP_BYTES // 2
    assert (np.diff(a) > 0).all()  # a sorted sample without repeats of the flat array (whose values are its indices)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) < 64 * 10**6
    bench.dump_outputs(str(tmp_path / "again"), {"big": big})  # alone, it may use the whole budget; same seed
    b = np.load(tmp_path / "again" / "big.npy")
    assert b.nbytes <= bench.DUMP_BYTES and (np.diff(b) > 0).all()
