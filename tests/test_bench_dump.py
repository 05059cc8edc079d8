"""bench.py --dump-outputs: the arrays of the last timed step as DIR/<name>.npy (float32 /
float64, at most bench.DUMP_BUDGET_BYTES in all, larger arrays as a fixed seeded sample), and
the plain / --full split of the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_sample_small_arrays_are_kept_whole():
    import bench
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    out = bench._dump_sample(a, 48)
    assert out.dtype == np.float32 and out.shape == (3, 4) and np.array_equal(out, a)
    i = bench._dump_sample(np.arange(5, dtype=np.int64), 1 << 10)
    assert i.dtype == np.float64 and np.array_equal(i, np.arange(5.0))
    h = bench._dump_sample(np.ones(3, dtype=np.float16), 1 << 10)
    assert h.dtype == np.float32


def test_dump_sample_large_arrays_are_a_fixed_sample():
    import bench
    a = np.random.default_rng(3).standard_normal(1000).astype(np.float32)
    s1, s2 = bench._dump_sample(a, 400), bench._dump_sample(a.copy(), 400)
    assert s1.dtype == np.float32 and s1.shape == (100,) and s1.nbytes <= 400
    assert np.array_equal(s1, s2)  # the same elements every run
    assert np.isin(s1, a).all() and not np.array_equal(s1, a[:100])


def test_full_and_dump_outputs_are_options():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout


@pytest.mark.gpu
def test_dump_outputs_writes_the_last_step(cuda, tmp_path):
    import bench
    g = torch.Generator().manual_seed(5)
    x = torch.cumsum(0.1 * torch.randn(16, 3, 64, generator=g), -1)
    x = 2 * (x - x.amin(0, keepdim=True)) / (x.amax(0, keepdim=True) - x.amin(0, keepdim=True) + 1e-8) - 1
    batch = (x.to(cuda), torch.randint(0, 5, (16, 1), generator=g).to(cuda))
    tr = bench.JointTrainer(cuda, 1, length=64, channels=3)
    tr.capture(batch)
    out1, out2 = tr.step(batch)
    torch.cuda.synchronize()
    bench.dump_outputs(str(tmp_path / "d"), tr, out1, out2)
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert {"stage1.loss", "stage2.loss", "stage1.params", "stage2.params",
            "stage1.buffers"} <= set(got)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES
    assert np.array_equal(got["stage1.params"], tr.opt1.flat.cpu().numpy())
    assert np.array_equal(got["stage2.params"], tr.opt2.flat.cpu().numpy())
    assert float(got["stage1.loss"].sum()) == float(out1["loss"].sum())
    assert float(got["stage2.loss"].sum()) == float(out2["loss"].sum())
    assert all(np.isfinite(a).all() for a in got.values())
