#!/usr/bin/env python3
"""What the per-effector rotation term costs: solve_track on the reference tree without the term (the
plain track kernel) and with orientation targets for all three effectors (ikpso_solve_track_frames,
weight 1), on the shape of tests/test_gpu_frames.py::test_it_steers -- 64 swarms x 1024 particles x 100
iterations, one frame, FAST, no stop -- and on a shape that fills the device.

The runs alternate in one process after warm-up, device events around each whole call, re-seeded
outside the timed region; the order rotates from repetition to repetition.  --package DIR imports the
ikpso package of another checkout (a build of the parent commit: only "plain" is timed there, on the
same inputs).  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
ap = argparse.ArgumentParser()
ap.add_argument("--swarms", type=int, default=64)
ap.add_argument("--iterations", type=int, default=100)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--package", default=str(ROOT / "inverse-kinematics-pso-research_amd"))
ap.add_argument("--out", default=str(ROOT / "profiles" / "frames" / "frames_timing.json"))
args = ap.parse_args()
sys.path.insert(0, args.package)
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch

import frames64
import ikpso
import topologies as tp

assert torch.cuda.is_available(), "frames_timing.py needs a GPU"
chain = ikpso.reference_scene(reset=True).origin.to_cuda()
B, P, I, E = args.swarms, 1024, args.iterations, 3
# reachable targets, as the tests draw them: the effector frames of random in-bounds joint vectors
theta = tp.random_poses(chain, B, np.random.default_rng([22, len(chain)]))
p, R = frames64.effector_frames(chain, theta)
tg = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32).reshape(1, B, E, 3)).cuda()
rot = torch.from_numpy(np.ascontiguousarray(R, dtype=np.float32).reshape(1, B, E, 3, 3)).cuda()

solver = ikpso.BatchSolver(chain, P, pso=ikpso.PSOConfig(0.5, 0.5, 1.25, I), kernel="resident")
RUNS = {"plain": lambda: solver.solve_track(tg, iterations=I)}
if "ikpso_solve_track_frames" in ikpso._abi.SIGNATURES:
    RUNS["frames"] = lambda: solver.solve_track(tg, iterations=I, effector_rot=rot, effector_rot_weight=1.0)


def timed(run):
    solver.seed(B)
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = run()
    z.record()
    z.synchronize()
    return a.elapsed_time(z), out


names = list(RUNS)
times, kernels = {n: [] for n in names}, {}
for k in range(args.warmup + args.reps):
    r = k % len(names)
    for name in names[r:] + names[:r]:
        ms, out = timed(RUNS[name])
        kernels[name] = solver.kernel
        if k >= args.warmup:
            times[name].append(ms)
        elif k == 0:
            assert bool(torch.isfinite(out[1]).all()) and bool((out[3] == I).all()), name


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "runs": len(ts)}


result = {"workload": f"reference tree, {B} swarms x {P} particles, 1 frame x {I} iterations, FAST, no stop",
          "package": os.path.relpath(args.package, ROOT), "kernels": kernels}
result.update({n: stats(times[n]) for n in names})
if "frames" in times:
    result["ratio_frames_over_plain"] = result["frames"]["median_ms"] / result["plain"]["median_ms"]
print(json.dumps(result))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
