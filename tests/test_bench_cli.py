"""bench.py's command line: a plain run measures the headline only, --full is where everything else lives,
--steps is the number of timed steps, --dump-outputs writes what the timed path computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("laplacian_only", "mfma_variant", "roofline_hbm", "weak_hbm", "velocity_solve", "cpu_baseline",
             "speedup_vs_cpu")


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_options(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (20, 5, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    y = torch.arange(5000, dtype=torch.float64) * 0.5
    bench.dump_outputs(str(tmp_path / "a"), y, 1, 0)
    got = np.load(tmp_path / "a" / "y.npy")
    assert got.dtype == np.float64 and np.array_equal(got, y.numpy())
    # an output beyond the limit: a sample at the same increasing positions in every run, within each rank's share
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 16384)
    for d in ("b", "c"):
        for rank in (0, 1):
            bench.dump_outputs(str(tmp_path / d), y + rank, 2, rank)
    files = sorted(os.listdir(tmp_path / "b"))
    assert files == ["y_rank0.npy", "y_rank1.npy"]
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in files) <= 16384
    b0, b1, c0 = (np.load(tmp_path / d / f) for d, f in (("b", files[0]), ("b", files[1]), ("c", files[0])))
    assert np.array_equal(b0, c0) and np.array_equal(b1, b0 + 1)
    assert 900 < b0.size < 5000 and np.all(np.diff(b0) > 0) and np.all(np.isin(b0, y.numpy()))


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path, gpu):
    """The plain command: --steps timed steps, the headline keys, nothing that needs a run of its own; y.npy is
    bitwise the apply of the same seeded inputs."""
    import bench
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert "graph1000_us" not in line["roofline"]
    assert line["steps"] == 7 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["unit"] == "DOF-updates/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    n = line["config"]["dofs_global"]
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] * 1e-3), rel=1e-12)
    assert os.listdir(out) == ["y.npy"]
    y = np.load(out / "y.npy")
    assert y.dtype == np.float64 and y.shape == (n,)
    step, _, (_, want, _), _ = bench.build_strip_step(8, 64, 64, 1.0 / 64, 40.0, 1, 0, gpu, None, seed=2024)
    step()
    torch.cuda.synchronize(gpu)
    assert np.array_equal(y, want.cpu().numpy())
