"""Aim targets on the GPU: BatchSolver.solve_track / solve_until with aim_dir (ikpso_solve_track_aim),
the folded chain's track kernels with the tool-axis term w |R_eff a - d|^2, the roll about a free.

The oracle has no such term, so the checkers are those of tests/test_gpu_pose.py: the existing
solve_track (weight 0 must equal it bit for bit), a loop of one-frame aim calls (the frame
contract), the fitness recomputed in numpy float64 from the node table and the definition
(tests/aim64.py), and for "does it steer" the weight-0 run itself -- the parent's behaviour -- under
tests/tierb.py's strict paired sign test.

Targets are the float64 poses of random in-bounds joint vectors with d = R a of the same vector, so
every target is reachable.  The axis is (1, 2, 3) / sqrt(14): all three components of a' matter.
"""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aim64
import ikpso
import pose64
import tierb
import topologies as tp
from ikpso.dh import iiwa14

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, T, IT = 8, 3, 30
SIZES = (65, 1024)  # a second wave with one lane; the full workgroup
ARMS = ("dh3", "dh7", "dh12", "iiwa14")
AXIS = (1.0, 2.0, 3.0)  # handed over un-normalised: the library normalises
ALPHA = 0.01            # tests/tierb.py stat_tests' level
OK, UNSUPPORTED, INVALID = ikpso._abi.IKPSO_OK, ikpso._abi.IKPSO_ERR_UNSUPPORTED, ikpso._abi.IKPSO_ERR_INVALID_ARG
# The fitness bound REL * want + FLOOR, restated from tests/test_gpu_pose.py (the same kernel family
# with a larger term, |R - T|_F^2 <= 8 there against |R a - d|^2 <= 4 here): the FAST tolerance on a
# fitness (tests/tierb.py TOLS, rel_fitness) plus that file's absolute floor 4 x 1.476e-6.
REL = dict(tierb.TOLS)["rel_fitness"]
FLOOR = 4 * 1.476e-6


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Case:
    """An arm, its axis mask, its fitness configuration and B x T reachable aim targets."""

    def __init__(self, name, nb=B, frames=T, seed=11, axis=AXIS):
        self.name = name
        if name == "iiwa14":
            self.arm, self.fit = iiwa14(), ikpso.FitnessConfig(0.0, 0.0, 0.1)  # the dh7 workload's
        else:
            self.arm, self.fit = tp.dh_arm_n(int(name[2:]))[0], ikpso.MAIN_FITNESS
        self.chain, self.mask = self.arm.origin.to_cuda(), self.arm.axis_mask
        rng = np.random.default_rng([seed, len(self.chain)])
        self.theta = tp.random_poses(self.chain, nb * frames, rng, self.mask)
        p, R = pose64.poses(self.chain, self.theta, self.mask)
        self.axis = tuple(float(v) for v in axis)
        self.R = R
        self.targets = p.astype(np.float32).reshape(frames, nb, 1, 3)
        self.dirs = (R @ aim64.unit(axis)).astype(np.float32).reshape(frames, nb, 3)

    def solver(self, P, iterations=IT, **kw):
        kw.setdefault("kernel", "resident")
        kw.setdefault("axis_mask", self.mask)
        return ikpso.BatchSolver(self.chain, P, pso=ikpso.PSOConfig(0.5, 0.5, 1.25, iterations), fit=self.fit, **kw)


@pytest.fixture(scope="module")
def cases(device):
    out = {name: Case(name) for name in ARMS}
    # the real arm once more with the tool z axis, named in the DH tool frame
    out["iiwa14-tool-z"] = Case("iiwa14", axis=iiwa14().node_axis((0.0, 0.0, 1.0)))
    return out


NAMES = ARMS + ("iiwa14-tool-z",)


def run_track(case, P, stop=None, iterations=IT, **aim):
    """solve_track on a fresh solver: [angles, fitness, residual, iterations, states], kernel name.
    aim: weight=... runs the aim entry with the case's directions."""
    s = case.solver(P, iterations)
    nb = case.targets.shape[1]
    s.seed(nb)
    kw = {}
    if "weight" in aim:
        kw = dict(aim_dir=dev(case.dirs), aim_axis=case.axis, aim_weight=aim["weight"])
    out = [t.cpu().numpy() for t in s.solve_track(dev(case.targets), iterations=iterations, stop_fitness=stop, **kw)]
    out.append(s.generator_states(0, nb))
    name = s.kernel
    s.close()
    return out, name


def run_loop(case, P, stop, weight, iterations=IT):
    """The frame contract's checker: one frames = 1 aim call (solve_until) per frame on a fresh
    solver, each fed the previous answers.  Also the generator states after frame 0."""
    s = case.solver(P, iterations)
    nb = case.targets.shape[1]
    s.seed(nb)
    frames, prev, first_states = [[], [], [], []], None, None
    for t in range(case.targets.shape[0]):
        out = s.solve_until(dev(case.targets[t]), start_pose=prev, max_iterations=iterations,
                            stop_fitness=-1.0 if stop is None else stop, aim_dir=dev(case.dirs[t]),
                            aim_axis=case.axis, aim_weight=weight)
        prev = out[0]
        for acc, o in zip(frames, out):
            acc.append(o.cpu().numpy())
        if t == 0:
            first_states = s.generator_states(0, nb)
    out = [np.stack(f) for f in frames]
    out.append(s.generator_states(0, nb))
    s.close()
    return out, first_states


def assert_same(got, want):
    for name, g, w in zip(("angles", "fitness", "residual", "iterations", "generator states"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(bits(g), bits(w)), (name, np.argwhere(bits(g) != bits(w))[:8].tolist())


# ------------------------------------------------------------------ 5. weight zero is today's track
@pytest.mark.parametrize("stopping", [False, True], ids=["never-stops", "median-stop"])
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("name", ARMS)
def test_weight_zero_is_solve_track(cases, name, P, stopping):
    """Weight 0 is the term absent (the entry then runs the track kernel without it): bit for bit the
    call without aim_dir -- angles, fitness, residual, iteration counts and generator states."""
    case = cases[name]
    plain, kname = run_track(case, P)
    assert f"swarm_resident<dh{case.arm.joints}>" in kname, kname
    stop = float(np.median(plain[1])) if stopping else None  # (from the checker: the call without aim_dir)
    want = run_track(case, P, stop)[0] if stopping else plain
    got, _ = run_track(case, P, stop, weight=0.0)
    assert_same(got, want)
    if stopping:
        assert (want[3] < IT).any() and (want[3] == IT).any(), want[3].tolist()


# ------------------------------------------------------------ 6. the fitness is what the header says
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_fitness_is_what_the_header_says(cases, name, P):
    case = cases[name]
    (ang, fit, res, its, _), kname = run_track(case, P, weight=1.0)
    assert f"swarm_resident<dh{case.arm.joints}>" in kname, kname
    assert (its == IT).all()
    D = ang.shape[2]
    start = np.array([case.chain["rotation"][k][c] for k, c in tp.free_axes(case.chain, case.mask)], np.float32)
    rest = np.concatenate([np.broadcast_to(start, (1, B, D)), ang[:-1]])  # frame t starts from frame t-1's answer
    want = aim64.aim_fitness(case.chain, case.mask, case.fit.angle_weight, ang.reshape(-1, D), rest.reshape(-1, D),
                             case.targets, case.axis, case.dirs, 1.0).reshape(T, B)
    err = np.abs(fit.astype(np.float64) - want)
    small = want < FLOOR / REL
    print(f"{name} P={P}: fitness {want.min():.3e}..{want.max():.3e}, max |gpu - float64| = {err.max():.3e}, "
          f"max relative {np.max(err / want):.3e}, max absolute where the floor decides "
          f"{err[small].max() if small.any() else 0.0:.3e}")
    assert np.isfinite(fit).all()
    assert (err <= REL * want + FLOOR).all(), (err.max(), np.argwhere(err > REL * want + FLOOR)[:4].tolist())
    # the residual stays the positional checkDistance residual
    p, _ = pose64.poses(case.chain, ang.reshape(-1, D), case.mask)
    want_res = np.linalg.norm(p - case.targets.reshape(-1, 3).astype(np.float64), axis=1).reshape(T, B)
    assert np.max(np.abs(res - want_res)) <= 1e-4, np.max(np.abs(res - want_res))


# -------------------------------------------------------------------------------- 7. the frame loop
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("name", ARMS)
def test_frame_loop(cases, name, P):
    case = cases[name]
    # the threshold as tests/test_gpu_track.py's median_threshold takes it: the median fitness of a
    # never-stopping checker loop
    stop = float(np.median(run_loop(case, P, None, 1.0)[0][1]))
    want, first_states = run_loop(case, P, stop, 1.0)
    got, _ = run_track(case, P, stop, weight=1.0)
    print("iterations:", got[3].tolist())
    assert_same(got, want)
    n = want[3]
    assert (n < IT).any() and (n == IT).any(), n.tolist()
    assert (want[1][n < IT] <= stop).all() and (want[1][n == IT] > stop).sum() > 0
    # a frame that stopped at n is a never-stopping call of n iterations: frame 0, by count
    for count in sorted(set(n[0].tolist()) - {IT}):
        s = case.solver(P, IT)
        s.seed(B)
        out = [t.cpu().numpy() for t in s.solve_until(dev(case.targets[0]), max_iterations=count, stop_fitness=-1.0,
                                                      aim_dir=dev(case.dirs[0]), aim_axis=case.axis, aim_weight=1.0)]
        states = s.generator_states(0, B).reshape(B, P, -1)
        s.close()
        rows = n[0] == count
        assert (out[3] == count).all()
        for k, label in enumerate(("angles", "fitness", "residual")):
            assert np.array_equal(bits(out[k][rows]), bits(want[k][0][rows])), (label, count)
        assert np.array_equal(states[rows], first_states.reshape(B, P, -1)[rows]), count


# ------------------------------------------------------------- 8. it steers; 9. the roll is free
def sign_test_smaller(x, y):
    """tests/tierb.py's strict paired sign test (only exactly equal values tie), H0 "x is as likely
    to be larger than y as smaller" against "smaller": (smaller, larger, p)."""
    from scipy.stats import binomtest

    smaller, larger = int(np.sum(x < y)), int(np.sum(x > y))
    assert tierb.SIGN_TIE == 0.0
    p = float(binomtest(smaller, smaller + larger, 0.5, alternative="greater").pvalue) if smaller + larger else 1.0
    return smaller, larger, p


@pytest.fixture(scope="module")
def steering(device):
    """iiwa, 64 swarms x 1024 particles x 100 iterations, one frame, the same seeds: the tool z axis
    (through DHArm.node_axis) held along d at aim weight 1, against weight 0, and against the pose
    entry at weight 1 on full pose targets built from an arbitrary roll about the axis."""
    nb, P, iters = 64, 1024, 100
    arm = iiwa14()
    case = Case("iiwa14", nb=nb, frames=1, seed=12, axis=arm.node_axis((0.0, 0.0, 1.0)))
    a = aim64.unit(case.axis)
    psi = np.random.default_rng(13).uniform(-np.pi, np.pi, nb)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    roll = np.eye(3) + np.sin(psi)[:, None, None] * K + (1.0 - np.cos(psi))[:, None, None] * (K @ K)  # Rot(a, psi)
    rolled = case.R @ roll
    assert np.max(np.abs(rolled @ a - case.R @ a)) <= 1e-12  # the same tool axis, another roll
    runs = {}
    for key, kw in (("aim", dict(aim_dir=dev(case.dirs[0]), aim_axis=case.axis, aim_weight=1.0)),
                    ("none", dict(aim_dir=dev(case.dirs[0]), aim_axis=case.axis, aim_weight=0.0)),
                    ("pose", dict(target_rot=dev(rolled.astype(np.float32)), orientation_weight=1.0))):
        s = case.solver(P, iters)
        s.seed(nb)
        runs[key] = [t.cpu().numpy() for t in s.solve_until(dev(case.targets[0]), max_iterations=iters,
                                                            stop_fitness=-1.0, **kw)]
        s.close()
    return case, runs


def test_it_steers(steering):
    case, runs = steering
    ang = {k: aim64.aim_angle(pose64.poses(case.chain, runs[k][0], case.mask)[1], case.axis, case.dirs[0])
           for k in ("aim", "none")}
    smaller, larger, p = sign_test_smaller(ang["aim"], ang["none"])
    print(f"angle between the tool axis and d, median: weight 1 {np.median(ang['aim']):.4e} rad, weight 0 "
          f"{np.median(ang['none']):.4e} rad; residual, median: weight 1 {np.median(runs['aim'][2]):.4e}, weight 0 "
          f"{np.median(runs['none'][2]):.4e}; smaller in {smaller} of 64, larger in {larger}, p = {p:.3e}")
    assert len(ang["aim"]) == 64 and p < ALPHA, (smaller, larger, p)


def test_the_roll_is_free(steering):
    """What the entry adds over ikpso_solve_track_pose: a caller who must invent a roll gives up a
    degree of freedom, and the positional residual pays for it."""
    case, runs = steering
    smaller, larger, p = sign_test_smaller(runs["aim"][2], runs["pose"][2])
    print(f"positional residual, median: aim {np.median(runs['aim'][2]):.4e}, pose with an arbitrary roll "
          f"{np.median(runs['pose'][2]):.4e}; aim smaller in {smaller} of 64, larger in {larger}, p = {p:.3e}")
    assert len(runs["aim"][2]) == 64 and p < ALPHA, (smaller, larger, p)


# ------------------------------------------------------------------ 10. refusals and bad arguments
def aim_status(s, case, weight=1.0, dirs=True, axis=AXIS, frames=1):
    """The C entry's status on device buffers of the right sizes (nothing is read back)."""
    import ctypes

    nb = case.targets.shape[1]
    tg, dr = dev(case.targets[:max(frames, 1)]), dev(case.dirs[:max(frames, 1)])
    ang = torch.empty((max(frames, 1), nb, s.dof), dtype=torch.float32, device="cuda")
    fit = torch.empty((max(frames, 1), nb), dtype=torch.float32, device="cuda")
    host_axis = None if axis is None else (ctypes.c_float * 3)(*axis)
    st = s._lib.ikpso_solve_track_aim(s._h, tg.data_ptr(), dr.data_ptr() if dirs else None, host_axis, float(weight),
                                      None, nb, frames, IT, -1.0, ang.data_ptr(), fit.data_ptr(), None, None, None)
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("how", ["reference", "nofold", "streaming", "coop", "unmasked"])
def test_unsupported_solvers(cases, how):
    case = cases["iiwa14"]
    if how == "unmasked":
        chain = ikpso.serial_chain(7, 0.5).to_cuda()
        s = ikpso.BatchSolver(chain, 128, kernel="resident")
    else:
        kw = {"reference": dict(arith="reference"), "nofold": dict(fold=False), "streaming": dict(kernel="streaming"),
              "coop": dict(kernel="coop")}[how]
        s = case.solver(1024 if how == "coop" else 128, **kw)
    s.seed(B)
    assert aim_status(s, case) == UNSUPPORTED
    assert aim_status(s, case, frames=0) == UNSUPPORTED  # before the empty call's IKPSO_OK
    if how != "unmasked":
        with pytest.raises(ikpso.IkpsoError) as e:
            s.solve_track(dev(case.targets), aim_dir=dev(case.dirs), aim_axis=AXIS, aim_weight=1.0)
        assert e.value.status == UNSUPPORTED
    s.close()


def test_invalid_arguments_and_empty_calls(cases):
    case = cases["iiwa14"]
    s = case.solver(128)
    s.seed(B)
    before = s.generator_states(0, B)
    nan, inf = float("nan"), float("inf")
    assert aim_status(s, case, weight=-1.0) == INVALID
    assert aim_status(s, case, weight=nan) == INVALID
    assert aim_status(s, case, dirs=False) == INVALID
    for axis in (None, (0.0, 0.0, 0.0), (nan, 0.0, 1.0), (0.0, inf, 0.0), (3e-7, 0.0, 0.0)):
        assert aim_status(s, case, axis=axis) == INVALID, axis
    lib = s._lib
    st = lib.ikpso_solve_track_aim(s._h, dev(case.targets[:1]).data_ptr(), None, None, 0.0, None, B, 1, IT, nan,
                                   None, None, None, None, None)
    assert st == INVALID  # a NaN stop_fitness
    assert np.array_equal(s.generator_states(0, B), before)
    assert aim_status(s, case, weight=0.0, dirs=False, axis=None) == OK  # weight 0 reads neither
    s.seed(B)
    assert aim_status(s, case, frames=0) == OK
    assert lib.ikpso_solve_track_aim(s._h, None, None, None, 0.0, None, B, 0, IT, -1.0, None, None, None, None,
                                     None) == OK
    tg = dev(case.targets)
    ang = torch.empty((T, B, s.dof), dtype=torch.float32, device="cuda")
    assert lib.ikpso_solve_track_aim(s._h, tg.data_ptr(), None, None, 0.0, None, 0, T, IT, -1.0, ang.data_ptr(), None,
                                     None, None, None) == OK  # num_swarms == 0
    # frames > 0 needs targets and out_angles, even with no swarm to solve
    st = lib.ikpso_solve_track_aim(s._h, None, None, None, 0.0, None, 0, T, IT, -1.0, None, None, None, None, None)
    assert st == INVALID
    assert np.array_equal(s.generator_states(0, B), before)  # no device work: the generators did not move
    with pytest.raises(ValueError):
        s.solve_track(tg, target_rot=dev(np.broadcast_to(np.eye(3, dtype=np.float32), (T, B, 3, 3))),
                      aim_dir=dev(case.dirs), aim_weight=1.0)
    with pytest.raises(ValueError):
        s.solve_until(tg[0], target_rot=dev(np.broadcast_to(np.eye(3, dtype=np.float32), (B, 3, 3))),
                      aim_dir=dev(case.dirs[0]), aim_weight=1.0)
    s.close()


# ------------------------------------------------------------------------------ 11. the C example
def test_aim_from_plain_c(device):
    exe = Path(__file__).resolve().parents[1] / "examples" / "_build" / "aim_c"
    if not exe.exists():
        pytest.fail(f"{exe} not built (__graft_entry__.build() builds examples/)")
    r = subprocess.run(["timeout", "-k", "10", "100", str(exe), "32", "100", "1"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "swarm_resident<dh7>" in r.stdout and "finite 1" in r.stdout, r.stdout
    rows = re.findall(r"frame (\d+): position error (\S+) m, aim error (\S+) rad \(weight 0: (\S+) m, (\S+) rad\)",
                      r.stdout)
    assert [int(x[0]) for x in rows] == [0, 1, 2, 3], r.stdout
    for _, _, angle, _, angle0 in rows:
        assert float(angle) < float(angle0), r.stdout
