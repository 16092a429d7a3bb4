"""bench.py's command line: a plain run measures the headline alone, --full adds
the other measurements, --dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]

FULL_ONLY = ("single_solve_ms", "reference_arith", "legs", "frame", "cpu_baseline", "speedup_vs_cpu")


def _bench_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("ikpso_bench", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_options(monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_splits_rows(tmp_path):
    bench = _bench_module()
    D = 21
    rows = np.arange(5 * (D + 2), dtype=np.float32).reshape(5, D + 2)
    bench.dump_outputs(str(tmp_path / "o"), rows, D)
    got = {p.name: np.load(p) for p in (tmp_path / "o").iterdir()}
    assert sorted(got) == ["angles.npy", "fitness.npy", "residual.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["angles.npy"], rows[:, :D])
    assert np.array_equal(got["fitness.npy"], rows[:, D])
    assert np.array_equal(got["residual.npy"], rows[:, D + 1])


def test_dump_outputs_samples_above_the_limit(tmp_path, monkeypatch):
    """Above the size limit: the same seeded, ascending sample of the swarms every time, its indices beside it."""
    bench = _bench_module()
    D = 3
    rows = np.random.default_rng(1).random((1000, D + 2)).astype(np.float32)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100 * (8 + 4 * (D + 2)))
    out = []
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), rows, D)
        out.append({p.name: np.load(p) for p in (tmp_path / name).iterdir()})
    a, b = out
    assert sorted(a) == ["angles.npy", "fitness.npy", "residual.npy", "swarm_index.npy"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["swarm_index.npy"]
    assert idx.dtype == np.float64 and idx.shape == (100,) and np.all(np.diff(idx) > 0)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES
    assert np.array_equal(a["angles.npy"], rows[idx.astype(np.int64), :D])
    assert np.array_equal(a["residual.npy"], rows[idx.astype(np.int64), D + 1])


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_last_step(tmp_path, device):
    """A plain run fills the headline and leaves every --full measurement out; the dumped arrays are the
    (warmup + steps)-th solve of the same seeded batch, bit for bit."""
    import torch

    import ikpso

    B, I, steps, warmup = 96, 20, 2, 1
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--swarms-per-gpu", str(B), "--iterations", str(I), "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == steps and rec["warmup"] == warmup and rec["full"] is False
    assert rec["ms_per_step"] > 0 and rec["unit"] == "particle-updates/s" and rec["dtype"] == "f32"
    assert rec["value"] == pytest.approx(B * 1024 * I / (rec["ms_per_step"] / 1e3), rel=1e-9)
    assert all(rec[k] is None for k in FULL_ONLY), {k: rec[k] for k in FULL_ONLY}

    wl = ikpso.workload(3)
    assert wl.particles == 1024
    s = ikpso.BatchSolver(wl.chain, wl.particles, pso=ikpso.PSOConfig(0.5, 0.5, 1.25, I), fit=wl.fit, arith="fast",
                          limit_weight=wl.limit_weight, soft_lo=wl.soft_lo, soft_hi=wl.soft_hi, kernel="auto",
                          axis_mask=wl.axis_mask, fold=wl.fold)
    s.seed(B, seed_base=0, first_swarm=0)
    tg = torch.from_numpy(wl.targets(0, B)).to(device)
    for _ in range(warmup + steps):
        ang, fit, res = (t.cpu().numpy() for t in s.solve(tg, iterations=I))
    s.close()
    assert np.array_equal(np.load(tmp_path / "out" / "angles.npy"), ang)
    assert np.array_equal(np.load(tmp_path / "out" / "fitness.npy"), fit)
    assert np.array_equal(np.load(tmp_path / "out" / "residual.npy"), res)
