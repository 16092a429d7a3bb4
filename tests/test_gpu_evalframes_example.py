"""examples/evalframes_c.c: ikpso_solver_evaluate_frames from plain C -- built by its Makefile rule and run
as tests/test_gpu_examples.py runs its examples, each step under its own time limit."""
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

EXAMPLES = Path(__file__).resolve().parents[1] / "examples"


def test_evalframes_from_plain_c(device):
    b = subprocess.run(["make", "-C", str(EXAMPLES), "_build/evalframes_c"], capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(EXAMPLES / "_build" / "evalframes_c"), "16", "100"], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr  # 3: the entry's fitness and the solve's disagree
    assert "kernel swarm_resident_frames<ref_tree7>" in r.stdout, r.stdout
    assert "finite 1 agree 1" in r.stdout, r.stdout
    rows = re.findall(r"wrist (\d+): angle to target (\S+) rad", r.stdout)
    assert [int(k) for k, _ in rows] == [0, 1, 2], r.stdout
    assert all(0.0 <= float(a) < 3.1416 for _, a in rows), r.stdout
