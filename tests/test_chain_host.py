"""The chain parser on the CPU: csrc/ikpso_chain.cpp (parse_chain, build_dh) linked into a
stand-alone program, every field of the parsed chains compared with a recording."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "inverse-kinematics-pso-research_amd" / "csrc"


def test_chain_parser_matches_golden(tmp_path, golden):
    """tests/host/chain_dump.cpp parses its fixed scenes -- each the smallest at which one branch
    of the parser can go wrong: topology and size, axis masks and the fold, bounds, soft limits,
    the distance term's slots, collider pruning and boxes -- and prints the status, whether the
    chain folded, and every field of both forms with floats as bit patterns.  The golden file
    was recorded from the parser as it stood inside ikpso_api.cpp, before it became a
    translation unit of its own; the output must equal it line for line."""
    exe = tmp_path / "chain_dump"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", f"-I{CSRC}",
                    f"-I{ROOT / 'include'}", str(ROOT / "tests" / "host" / "chain_dump.cpp"),
                    str(CSRC / "ikpso_chain.cpp"), "-o", str(exe)], check=True, capture_output=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    want = (golden / "chain_host.txt").read_text().splitlines()
    assert len(want) == 500
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}"
    assert len(got) == len(want)
