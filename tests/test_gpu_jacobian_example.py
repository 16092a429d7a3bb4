"""examples/jacobian_c.c: ikpso_solver_evaluate_jacobian from plain C -- built by its Makefile rule and run
as tests/test_gpu_evalframes_example.py runs its example, each step under its own time limit.  The
program is a demonstration (two Gauss-Newton steps on the host): only its exit status is held."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

EXAMPLES = Path(__file__).resolve().parents[1] / "examples"


def test_jacobian_from_plain_c(device):
    b = subprocess.run(["make", "-C", str(EXAMPLES), "_build/jacobian_c"], capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(EXAMPLES / "_build" / "jacobian_c"), "8", "100"], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
