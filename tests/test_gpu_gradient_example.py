"""examples/gradient_c.c: ikpso_solver_evaluate_gradient from plain C -- built by its Makefile rule and run as
tests/test_gpu_jacobian_example.py runs its example, each step under its own time limit.  The program
polishes PSO answers by projected gradient descent with a backtracking step that is accepted only if the
fitness decreases: no swarm's final fitness is above its starting one.  No convergence rate is asserted."""
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

EXAMPLES = Path(__file__).resolve().parents[1] / "examples"


def test_gradient_from_plain_c(device):
    b = subprocess.run(["make", "-C", str(EXAMPLES), "_build/gradient_c"], capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(EXAMPLES / "_build" / "gradient_c"), "8", "20", "40"], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    pairs = re.findall(r"^swarm \d+: fitness (\S+) -> (\S+)$", r.stdout, re.M)
    assert len(pairs) == 8
    for before, after in pairs:
        assert float(after) <= float(before)
