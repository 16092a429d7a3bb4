#!/usr/bin/env python3
"""Records tests/golden/resident_unroll.npz: what the resident FAST kernel of the reference
scene returns, byte for byte, for the cases of tests/test_gpu_resident_unroll.py.

Run on an MI355X from the commit whose answers are to be kept (the fixture in the tree was
recorded at 4c25385, before the iteration loop was unrolled):

    python3 tests/golden/gen_resident_unroll.py [OUT.npz]

Per case (P particles, I iterations; B = 4 swarms, targets wl.targets(0, B), seed_base 0):
    ang_P{P}_I{I} [B, D] f32, fit_P{P}_I{I} [B] f32, res_P{P}_I{I} [B] f32
    rng_P{P}_I{I} [32] u8   SHA-256 of the generator states after the solve, the int32
                            [B * P, 12] array BatchSolver.generator_states returns (the raw
                            states of all cases are 1.6 MB; the digest compares the same bytes)
and the second of two consecutive solves on one solver at P = 1024, I = 3: *_second.
"""
import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "inverse-kinematics-pso-research_amd"))

import torch  # noqa: E402

import ikpso  # noqa: E402

B = 4
ITERATIONS = (0, 1, 2, 3, 5, 6, 11)
PARTICLES = (64, 65, 1024)
SECOND = (1024, 3)  # (P, I) of the two-consecutive-solves case


def digest(states):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(states).tobytes()).digest(), dtype=np.uint8)


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(__file__).with_name("resident_unroll.npz")
    wl = ikpso.workload(3)
    tg = torch.from_numpy(np.ascontiguousarray(wl.targets(0, B))).cuda()
    z = {}

    def put(tag, s, res):
        ang, fit, rs = (t.cpu().numpy() for t in res)
        z["ang_" + tag], z["fit_" + tag], z["res_" + tag] = ang, fit, rs
        z["rng_" + tag] = digest(s.generator_states(0, B))

    for P in PARTICLES:
        with ikpso.BatchSolver(wl.chain, P, pso=wl.pso, fit=wl.fit, kernel="resident") as s:
            for I in ITERATIONS:
                s.seed(B, seed_base=0)
                put(f"P{P}_I{I}", s, s.solve(tg, iterations=I))
                assert "resident" in s.kernel and "ref_tree7" in s.kernel, s.kernel
                z["kernel"] = np.frombuffer(s.kernel.encode(), dtype=np.uint8)
            if P == SECOND[0]:
                s.seed(B, seed_base=0)
                s.solve(tg, iterations=SECOND[1])
                put(f"P{P}_I{SECOND[1]}_second", s, s.solve(tg, iterations=SECOND[1]))
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **z)
    print(f"{out}: {len(z)} arrays, {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
