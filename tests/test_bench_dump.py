"""bench.py --dump-outputs: what the timed path returned in its last step, as float32 .npy files under a size budget, the same on
every run with the same arguments (seeded weights and noise), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sample", "l_sample", "logp", "logp_terminal", "mean", "sigma", "control")


def _sampler_like_output(B, T):
    """A dict laid out as VARSampler.sample returns it: per-step lists of views of one trajectory block."""
    g = torch.Generator().manual_seed(0)
    traj = torch.randn(T + 1, B, 3, 32, 32, generator=g)
    mean, control = torch.randn(T, B, 3, 32, 32, generator=g), torch.randn(T, B, 3, 32, 32, generator=g)
    logp, sigma = torch.randn(T, B, generator=g), torch.rand(T, B, generator=g)
    return traj, {"sample": traj[T], "l_sample": list(traj.unbind(0)), "logp": list(logp.unbind(0)), "logp_terminal": torch.zeros(B),
                  "mean": list(mean.unbind(0)), "sigma": [s.view(-1, 1, 1, 1) for s in sigma.unbind(0)],
                  "control": list(control.unbind(0)), "_ring_slot": (0, 0)}


@pytest.mark.parametrize("B", [32, 256])
def test_dump_outputs_budget_and_rows(tmp_path, B):
    """Under the budget every row is written; above it (B = 256 at T = 10 is ~100 MB) every array keeps the same seeded rows."""
    import bench
    T = 10
    traj, d = _sampler_like_output(B, T)
    info = bench.dump_outputs(d, str(tmp_path))
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(n + ".npy" for n in NAMES)
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64_000_000
    a = {n: np.load(tmp_path / (n + ".npy")) for n in NAMES}
    assert all(v.dtype == np.float32 for v in a.values())
    keep = a["sample"].shape[0]
    if B == 32:
        assert keep == B and info["batch_rows"] == "all"
        rows = np.arange(B)
    else:
        assert 0 < keep < B and info["batch_rows"].startswith(f"{keep} of {B}")
        rows = np.sort(np.random.default_rng(bench.DUMP_ROW_SEED).choice(B, keep, replace=False))
    assert np.array_equal(a["l_sample"], traj.numpy()[:, rows]) and np.array_equal(a["sample"], a["l_sample"][T])
    assert a["mean"].shape == a["control"].shape == (T, keep, 3, 32, 32) and a["sigma"].shape == (T, keep, 1, 1, 1)
    assert a["logp"].shape == (T, keep) and a["logp_terminal"].shape == (keep,)
    assert info["arrays"] == {n: list(v.shape) for n, v in a.items()}


def test_plain_run_leaves_the_other_legs_to_full(monkeypatch):
    """Without --full a run measures the headline alone (asking it for train steps is an error); with it every leg is on by
    default and the --no-* options still take legs out."""
    import bench
    legs = ("no_events", "no_edm", "no_small_batch", "no_eager_reference", "no_cpu_baseline")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    a = bench.parse_args()
    assert not a.full and all(getattr(a, k) for k in legs) and a.train_steps == 0
    assert (a.gpus, a.steps, a.warmup, a.batch, a.T) == (1, 4, 2, 256, 10)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "4", "--train-steps", "0", "--no-edm"])
    a = bench.parse_args()
    assert not a.full and all(getattr(a, k) for k in legs) and a.train_steps == 0
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "4", "--train-steps", "3"])
    with pytest.raises(SystemExit):
        bench.parse_args()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2", "--full"])
    a = bench.parse_args()
    assert a.full and not any(getattr(a, k) for k in legs) and a.train_steps == 8
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-edm", "--train-steps", "0"])
    a = bench.parse_args()
    assert a.no_edm and not a.no_events and a.train_steps == 0


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_identically(tmp_path):
    """Two runs with the same arguments: --steps timed steps, ms_per_step in the line, and bit-identical dumps of the last step
    (the generation path reduces in a fixed order).  A run with one timed step fewer dumps another sample: what is written is
    the last timed step's output, not a warm-up's (noise is drawn inside every step)."""
    lines, dumps = [], []
    for run, steps in (("a", 3), ("b", 3), ("c", 2)):
        out = tmp_path / run
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", "32", "--train-steps", "0",
                            "--no-cpu-baseline", "--no-eager-reference", "--no-edm", "--no-events", "--no-small-batch", "--dump-outputs", str(out)],
                           cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        lines.append(json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1]))
        dumps.append({n: np.load(out / (n + ".npy")) for n in NAMES})
    for line, steps in zip(lines, (3, 3, 2)):
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["dump_outputs"]["batch_rows"] == "all"
        assert abs(line["value"] - 32 * steps / (line["ms_per_step"] * steps * 1e-3)) < 1e-6 * line["value"]
    a, b, c = dumps
    assert not np.array_equal(a["sample"], c["sample"]) and not np.array_equal(a["l_sample"][0], c["l_sample"][0])
    assert a["sample"].shape == (32, 3, 32, 32) and a["l_sample"].shape == (11, 32, 3, 32, 32)
    assert np.isfinite(a["sample"]).all() and np.array_equal(a["sample"], a["l_sample"][-1]) and a["sample"].std() > 0
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
