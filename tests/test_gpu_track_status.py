"""The status ladder of the four track entries (ikpso_solve_track, _pose, _aim, _frames), called through
the ABI: which status a call gets when more than one thing is wrong with it.  Every invalid argument
comes first, then a solver the entry does not serve, then the empty call (DESIGN, "The track entries'
status ladder").

Each row pairs the entry with a solver and one change to an otherwise good call.  The expected statuses
are what the build before the entries were folded onto one helper returned for the same rows (recorded
there, kept as literals), so the test holds the fold to that behaviour, not to its own.

No row reaches a kernel: every one is refused or empty, and the solvers are never seeded, so a row that
slipped through would be refused by the capacity check (IKPSO_ERR_INVALID_ARG) before any launch.
"""
import ctypes
import math

import pytest

import ikpso
import topologies as tp
from ikpso.dh import dh_arm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK, UNSUPPORTED, INVALID = ikpso._abi.IKPSO_OK, ikpso._abi.IKPSO_ERR_UNSUPPORTED, ikpso._abi.IKPSO_ERR_INVALID_ARG
P, B, T, IT = 64, 2, 2, 5
NAN, INF = float("nan"), float("inf")


def make_solvers():
    """fold3: a 3-joint masked serial chain that folds (serves pose and aim, not frames); plain2: a
    2-joint unmasked chain (serves frames, not pose or aim); ref2: the same chain with REFERENCE
    arithmetic (serves the plain entry alone)."""
    pso = ikpso.PSOConfig(0.5, 0.5, 1.25, IT)
    arm = dh_arm([0.3, 0.3, 0.2], [math.pi / 2, 0.0, 0.0], [0.0, 0.0, 0.0], [-2.0] * 3, [2.0] * 3)
    return {
        "fold3": ikpso.BatchSolver(arm.origin.to_cuda(), P, pso=pso, kernel="resident", axis_mask=arm.axis_mask),
        "plain2": ikpso.BatchSolver(tp.serial(2), P, pso=pso, kernel="resident"),
        "ref2": ikpso.BatchSolver(tp.serial(2), P, pso=pso, kernel="resident", arith="reference"),
    }


def call(entry, s, **change):
    """The status of `entry` on solver `s`: a good call of B swarms x T frames with `change` applied
    (a tensor argument set to None goes as a null pointer)."""
    E = s.effectors

    def z(*shape):
        return torch.zeros(shape, dtype=torch.float32, device="cuda")

    a = dict(targets=z(T, B, E, 3), rot=z(T, B, 3, 3), dirs=z(T, B, 3), eff_rot=z(T, B, E, 3, 3),
             axis=(0.0, 0.0, 1.0), weight=1.0, weights=[1.0] * E, nb=B, frames=T, stop=-1.0,
             angles=z(T, B, s.dof))
    a.update(change)

    def ptr(name):
        return None if a[name] is None else a[name].data_ptr()

    def host(name):
        return None if a[name] is None else (ctypes.c_float * len(a[name]))(*a[name])

    term = {"ikpso_solve_track": (),
            "ikpso_solve_track_pose": (ptr("rot"), a["weight"]),
            "ikpso_solve_track_aim": (ptr("dirs"), host("axis"), a["weight"]),
            "ikpso_solve_track_frames": (ptr("eff_rot"), host("weights"))}[entry]
    return getattr(s._lib, entry)(s._h, ptr("targets"), *term, None, a["nb"], a["frames"], IT, a["stop"],
                                  ptr("angles"), None, None, None, None)


TRACK, POSE, AIM, FRAMES = ("ikpso_solve_track", "ikpso_solve_track_pose", "ikpso_solve_track_aim",
                            "ikpso_solve_track_frames")
# (entry, solver, change, status of the build before the fold)
ROWS = [
    # the plain entry serves all three solvers: bad arguments, then the empty calls
    (TRACK, "ref2", dict(frames=-1), INVALID),
    (TRACK, "plain2", dict(stop=NAN), INVALID),
    (TRACK, "fold3", dict(nb=-1), INVALID),
    (TRACK, "ref2", dict(targets=None), INVALID),
    (TRACK, "ref2", dict(targets=None, nb=0), INVALID),
    (TRACK, "ref2", dict(nb=0), OK),
    (TRACK, "fold3", dict(frames=0, targets=None, angles=None), OK),
    # pose: plain2 and ref2 are not served; an invalid argument still answers first
    (POSE, "plain2", dict(weight=-1.0), INVALID),
    (POSE, "ref2", dict(weight=NAN), INVALID),
    (POSE, "plain2", dict(rot=None), INVALID),
    (POSE, "plain2", dict(frames=-1), INVALID),
    (POSE, "ref2", dict(stop=NAN), INVALID),
    (POSE, "plain2", dict(angles=None), INVALID),
    (POSE, "plain2", dict(), UNSUPPORTED),
    (POSE, "ref2", dict(), UNSUPPORTED),
    (POSE, "plain2", dict(weight=0.0, rot=None), UNSUPPORTED),  # no weight-0 detour to the plain kernel
    (POSE, "plain2", dict(nb=0), UNSUPPORTED),  # refused before the empty call's return
    (POSE, "ref2", dict(frames=0), UNSUPPORTED),
    (POSE, "fold3", dict(nb=0), OK),
    (POSE, "fold3", dict(frames=0, targets=None, angles=None), OK),
    (POSE, "fold3", dict(nb=0, weight=-1.0), INVALID),
    (POSE, "fold3", dict(nb=0, rot=None), INVALID),
    # aim: the pose entry's solvers; the axis is checked (and folded) before the refusal
    (AIM, "plain2", dict(weight=-1.0), INVALID),
    (AIM, "ref2", dict(weight=NAN), INVALID),
    (AIM, "plain2", dict(dirs=None), INVALID),
    (AIM, "plain2", dict(axis=None), INVALID),
    (AIM, "plain2", dict(axis=(0.0, 0.0, 0.0)), INVALID),
    (AIM, "ref2", dict(axis=(NAN, 0.0, 1.0)), INVALID),
    (AIM, "plain2", dict(frames=-1), INVALID),
    (AIM, "plain2", dict(targets=None), INVALID),
    (AIM, "plain2", dict(), UNSUPPORTED),
    (AIM, "ref2", dict(), UNSUPPORTED),
    (AIM, "plain2", dict(weight=0.0, axis=(0.0, 0.0, 0.0), dirs=None), UNSUPPORTED),  # weight 0 reads neither
    (AIM, "plain2", dict(nb=0), UNSUPPORTED),
    (AIM, "ref2", dict(frames=0), UNSUPPORTED),
    (AIM, "fold3", dict(nb=0), OK),
    (AIM, "fold3", dict(frames=0, targets=None, angles=None), OK),
    (AIM, "fold3", dict(nb=0, axis=(0.0, 0.0, 0.0)), INVALID),
    # frames: fold3 (masked) and ref2 (REFERENCE) are not served
    (FRAMES, "fold3", dict(weights=[-1.0]), INVALID),
    (FRAMES, "ref2", dict(weights=[NAN]), INVALID),
    (FRAMES, "fold3", dict(weights=[INF]), INVALID),
    (FRAMES, "fold3", dict(eff_rot=None), INVALID),
    (FRAMES, "ref2", dict(eff_rot=None), INVALID),
    (FRAMES, "fold3", dict(frames=-1), INVALID),
    (FRAMES, "ref2", dict(stop=NAN), INVALID),
    (FRAMES, "fold3", dict(angles=None), INVALID),
    (FRAMES, "fold3", dict(), UNSUPPORTED),
    (FRAMES, "ref2", dict(), UNSUPPORTED),
    (FRAMES, "fold3", dict(weights=None, eff_rot=None), UNSUPPORTED),  # no weight-0 detour either
    (FRAMES, "fold3", dict(nb=0), UNSUPPORTED),
    (FRAMES, "ref2", dict(frames=0), UNSUPPORTED),
    (FRAMES, "plain2", dict(nb=0), OK),
    (FRAMES, "plain2", dict(frames=0, targets=None, angles=None), OK),
    (FRAMES, "plain2", dict(nb=0, weights=[-1.0]), INVALID),
    (FRAMES, "plain2", dict(nb=0, eff_rot=None), INVALID),
]


def run_rows(solvers):
    """[(entry, solver, change, status)] of every row on `solvers`."""
    return [(entry, name, change, call(entry, solvers[name], **change)) for entry, name, change, _ in ROWS]


def test_track_entries_keep_their_status_ladder(device):
    solvers = make_solvers()
    try:
        assert solvers["fold3"].kernel.startswith("swarm_resident<dh3>"), solvers["fold3"].kernel
        got = run_rows(solvers)
    finally:
        for s in solvers.values():
            s.close()
    wrong = [(entry, name, change, status, want) for (entry, name, change, status), (_, _, _, want) in zip(got, ROWS)
             if status != want]
    assert not wrong, wrong
    assert {st for *_, st in got} == {OK, UNSUPPORTED, INVALID}  # the table reaches every rung
