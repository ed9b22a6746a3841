"""bench.py --dump-outputs: what the last timed step returned, written as DIR/<name>.npy in float32 / float64 within a
64 MB budget (larger outputs as a fixed, seeded sample), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_budget_dtypes_and_fixed_sample(tmp_path):
    import bench
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    arrays = {"big": big, "half": torch.linspace(-1, 1, 24, dtype=torch.bfloat16).reshape(2, 3, 4),
              "scal64": torch.tensor([1.5, -2.25], dtype=torch.float64), "idx": torch.arange(6).reshape(2, 3)}
    budget = 4096
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "half.npy", "idx.npy", "scal64.npy"]
    z = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert sum(a.nbytes for a in z.values()) <= budget
    assert z["scal64"].dtype == np.float64 and np.array_equal(z["scal64"], [1.5, -2.25])
    assert z["half"].dtype == np.float32 and z["half"].shape == (2, 3, 4)
    assert np.array_equal(z["half"], arrays["half"].float().numpy())
    assert z["idx"].dtype == np.float32 and np.array_equal(z["idx"], np.arange(6).reshape(2, 3))
    s = z["big"]                                       # sampled: 1-D, distinct sorted positions, the same every time
    assert s.dtype == np.float32 and s.ndim == 1 and 0 < s.size < big.numel()
    assert np.all(np.diff(s) > 0) and np.array_equal(s, np.floor(s))
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))


@pytest.mark.gpu
@pytest.mark.parametrize("workload, names", [
    ("train_step", ["head_losses", "sem_losses"]),
    ("infer", ["sem_argmax", "sem_out"]),
])
def test_bench_dump_outputs_run(tmp_path, workload, names):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
           "--size", "64", "--workload", workload, "--no-cpu-baseline", "--dump-outputs", out]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert "roofline" not in d and "cpu_baseline" not in d         # a plain run measures the headline figure alone
    assert sorted(os.listdir(out)) == [n + ".npy" for n in names]
    total = 0
    for n in names:
        a = np.load(os.path.join(out, n + ".npy"))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 << 20
    if workload == "infer":
        assert np.load(os.path.join(out, "sem_out.npy")).shape == (2, 2, 64, 64)
    else:
        assert np.load(os.path.join(out, "head_losses.npy")).shape == (4,)


@pytest.mark.gpu
def test_bench_full_adds_roofline_and_cpu_baseline():
    """--full: the same result line, with the objects whose measurements take runs of their own after the timed steps
    (the instrumented eager step and the CPU oracle)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
           "--size", "64", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    roof = d["roofline"]
    assert roof["launches_per_step"] > 0 and roof["achieved"] > 0 and roof["avg_launch_us"] > 0
    cpu = d["cpu_baseline"]
    assert cpu["value"] > 0 and cpu["unit"] == "images/s" and cpu["kind"] == "port"
    r = subprocess.run(cmd + ["--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert "roofline" in d and "cpu_baseline" not in d


def test_bench_options():
    """--full is off by default, and --no-cpu-baseline keeps its meaning under it (argument parsing alone: no GPU)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--no-cpu-baseline" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_bench_dump_outputs_repeat(tmp_path):
    """Two runs of the same command dump the same step: seeded random draws, and the last timed step restarted from the
    initial training state (otherwise float-atomic order and bf16 rounding let the trained weights drift apart within a
    few steps: the semantic losses of two runs differed by 40 %).  What remains is summation order inside the
    reductions, below one bf16 rounding (3.9e-3) of the stored activations."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dumps = []
    for i in range(2):
        out = str(tmp_path / str(i))
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2",
               "--size", "64", "--no-cpu-baseline", "--dump-outputs", out]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        dumps.append({n: np.load(os.path.join(out, n + ".npy")) for n in ("sem_losses", "head_losses")})
    a, b = dumps
    for name, tol in (("sem_losses", 1e-3), ("head_losses", 1e-2)):
        assert np.abs(a[name] - b[name]).max() <= tol * np.abs(a[name]).max(), (name, a[name], b[name])
