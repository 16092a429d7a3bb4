"""examples/track_c: ikpso_solve_track from plain C, compared by the example itself with the
loop of ikpso_solve_batch_until calls it replaces."""
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

EXE = Path(__file__).resolve().parents[1] / "examples" / "_build" / "track_c"


def test_track_from_plain_c(device):
    if not EXE.exists():
        pytest.fail(f"{EXE} not built (__graft_entry__.build() builds examples/)")
    r = subprocess.run([str(EXE), "32", "8", "15", "0.05"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "swarm_resident<ref_tree7>" in r.stdout, r.stdout
    assert "32 arms x 8 frames" in r.stdout and "finite 1" in r.stdout and "matches loop 1" in r.stdout, r.stdout
    its = float(re.search(r"mean iterations per frame ([0-9.]+)", r.stdout).group(1))
    assert 0.0 <= its <= 15.0
