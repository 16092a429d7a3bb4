#!/usr/bin/env python3
"""What the tool-axis (aim) term costs: solve_track without an orientation term, with pose targets
(ikpso_solve_track_pose, weight 1) and with aim targets (ikpso_solve_track_aim, weight 1), on the dh7
workload's shape -- the KUKA iiwa, 4096 swarms x 1024 particles, FAST, T frames of a fixed
iteration count, no stop.

The three alternate in one process after warm-up, device events around each whole call, re-seeded
outside the timed region; the order rotates from repetition to repetition.  Prints one JSON line
and writes it to --out."""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "inverse-kinematics-pso-research_amd"))
import numpy as np
import torch

import ikpso
from ikpso.dh import IIWA14, dh_forward_pose, iiwa14
from ikpso.workloads import splitmix64_stream, unit_floats

ap = argparse.ArgumentParser()
ap.add_argument("--swarms", type=int, default=4096)
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--iterations", type=int, default=125)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=str(ROOT / "profiles" / "aim" / "aim_timing.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "aim_timing.py needs a GPU"

wl = ikpso.workload("dh7")
arm = iiwa14()
B, P, T, I = args.swarms, wl.particles, args.frames, args.iterations
# reachable waypoints (tools/pose_timing.py's): the tool poses of joint vectors drawn as the workload's
# targets are; the aim direction is each pose's own tool z axis
u = unit_floats(splitmix64_stream(np.uint64(0x5EED7000) + np.arange(T * B, dtype=np.uint64), 7))
theta = (2.0 * u - 1.0) * 0.8 * IIWA14["limits"][None]
tool = np.array([dh_forward_pose(t, IIWA14["d"], IIWA14["a"], IIWA14["alpha"]) for t in theta])
tg = torch.from_numpy(tool[:, :3, 3].astype(np.float32).reshape(T, B, 1, 3)).cuda()
rot = torch.from_numpy(arm.node_target(tool[:, :3, :3]).astype(np.float32).reshape(T, B, 3, 3)).cuda()
dirs = torch.from_numpy(np.ascontiguousarray(tool[:, :3, 2]).astype(np.float32).reshape(T, B, 3)).cuda()
axis = arm.node_axis((0.0, 0.0, 1.0))

solver = ikpso.BatchSolver(wl.chain, P, pso=wl.pso, fit=wl.fit, axis_mask=wl.axis_mask, kernel="resident")
RUNS = {
    "plain": lambda: solver.solve_track(tg, iterations=I),
    "pose": lambda: solver.solve_track(tg, iterations=I, target_rot=rot, orientation_weight=1.0),
    "aim": lambda: solver.solve_track(tg, iterations=I, aim_dir=dirs, aim_axis=axis, aim_weight=1.0),
}


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
times = {n: [] for n in names}
for k in range(args.warmup + args.reps):
    for name in names[k % 3:] + names[:k % 3]:
        ms, out = timed(RUNS[name])
        if k >= args.warmup:
            times[name].append(ms)
        elif k == 0:
            assert bool(torch.isfinite(out[1]).all()) and bool((out[3] == I).all()), name


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "runs": len(ts)}


med = {n: float(np.median(times[n])) for n in names}
result = {"workload": f"dh7 (iiwa14), {B} swarms x {P} particles, {T} frames x {I} iterations, FAST, no stop",
          "kernel": solver.kernel, "plain": stats(times["plain"]), "pose": stats(times["pose"]),
          "aim": stats(times["aim"]), "ratio_pose_over_plain": med["pose"] / med["plain"],
          "ratio_aim_over_plain": med["aim"] / med["plain"], "ratio_aim_over_pose": med["aim"] / med["pose"],
          "updates_per_s_aim": B * P * T * I / (med["aim"] * 1e-3)}
print(json.dumps(result))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
