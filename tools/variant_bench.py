#!/usr/bin/env python3
"""Time several builds of libikpso.so on the bench workload, interleaved in ONE
process (rounds x variants), so clock/DVFS drift hits every variant alike.
usage: variant_bench.py LIB [LIB...] [--swarms N] [--rounds R] [--iters I]"""
import argparse
import ctypes
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "inverse-kinematics-pso-research_amd"))

import numpy as np
import torch

import ikpso
from ikpso import _abi


def open_lib(path):
    lib = ctypes.CDLL(str(path))
    for name, (res, args) in _abi.SIGNATURES.items():
        fn = getattr(lib, name, None)  # (an older build may lack a newer introspection entry)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def make_solver(lib, wl, P, I, arith="fast", kernel=0):
    """ikpso_solver_create through `lib` for workload `wl`; returns (handle, arrays to keep alive)."""
    desc = _abi.SolverDesc()
    chain = np.ascontiguousarray(wl.chain)
    desc.chain = chain.ctypes.data
    desc.node_count = chain.shape[0]
    desc.particles = P
    desc.pso = _abi.PSOConfig(0.5, 0.5, 1.25, I)
    desc.fit = wl.fit.c()
    desc.arith = 0 if arith == "fast" else 1
    desc.kernel = kernel
    keep = [chain]
    if wl.axis_mask is not None:
        m = np.ascontiguousarray(wl.axis_mask, np.uint8)
        keep.append(m)
        desc.axis_mask = m.ctypes.data
        desc.flags = 0 if wl.fold else _abi.FLAG_NO_FOLD
    if wl.limit_weight:
        lo = np.ascontiguousarray(wl.soft_lo, np.float32)
        hi = np.ascontiguousarray(wl.soft_hi, np.float32)
        keep += [lo, hi]
        desc.limit_weight = wl.limit_weight
        desc.soft_lo, desc.soft_hi = lo.ctypes.data, hi.ctypes.data
    h = ctypes.c_void_p()
    assert lib.ikpso_solver_create(ctypes.byref(desc), ctypes.byref(h)) == 0
    return h, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--swarms", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--arith", default="fast")
    ap.add_argument("--config", default="3", choices=["3", "5", "dh7"])
    ap.add_argument("--particles", type=int, default=0, help="override the workload's swarm size")
    ap.add_argument("--kernel", type=int, default=0, help="ikpso_solver_desc.kernel (0 = AUTO)")
    a = ap.parse_args()
    wl = ikpso.workload(int(a.config) if a.config.isdigit() else a.config)
    P, I, B = a.particles or wl.particles, a.iters, a.swarms
    D = wl.dof
    tg = torch.from_numpy(np.ascontiguousarray(wl.targets(0, B))).cuda()
    outs = [torch.empty((B, D), device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda")]
    solvers = []
    for p in a.libs:
        lib = open_lib(p)
        h, keep = make_solver(lib, wl, P, I, a.arith, a.kernel)
        assert lib.ikpso_solver_seed(h, B, 0, 0, None) == 0
        solvers.append((p, lib, h, keep))
    times = {p: [] for p in a.libs}
    results = {}
    for r in range(a.rounds + 1):
        for p, lib, h, _ in solvers:
            assert lib.ikpso_solver_seed(h, B, 0, 0, None) == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert lib.ikpso_solve_batch(h, tg.data_ptr(), None, B, I, outs[0].data_ptr(), outs[1].data_ptr(),
                                         outs[2].data_ptr(), None) == 0
            e1.record()
            assert lib.ikpso_solver_sync(h) == 0  # settles a cooperative solve (the timing build reports here)
            torch.cuda.synchronize()
            if r:
                times[p].append(e0.elapsed_time(e1))
            results[p] = float(outs[1].mean())
    for p in a.libs:
        t = np.array(times[p])
        ups = B * P * I / (np.median(t) / 1e3)
        print(f"{Path(p).name:40s} median {np.median(t):8.3f} ms  min {t.min():8.3f}  max {t.max():8.3f}  "
              f"spread {t.max() - t.min():6.3f}  {ups:.3e} upd/s  mean_fit {results[p]:.6f}")


if __name__ == "__main__":
    main()
