"""Pose targets on the GPU: BatchSolver.solve_track / solve_until with target_rot
(ikpso_solve_track_pose), the folded chain's track kernels with the tip orientation term.

The oracle has no orientation term, so the checkers are: the existing solve_track (weight 0 must
equal it bit for bit), a loop of one-frame pose calls (the frame contract), the fitness recomputed
in numpy float64 from the node table and the definition (tests/pose64.py), and for "does it steer"
the weight-0 run itself -- the parent's behaviour -- under tests/tierb.py's strict paired sign test.

Targets are the float64 poses of random in-bounds joint vectors, so every one is reachable.
"""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ikpso
import pose64
import tierb
import topologies as tp
from ikpso.dh import IIWA14, dh_forward_pose, iiwa14

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, T, IT = 8, 3, 30
SIZES = (65, 1024)  # a second wave with one lane; the full workgroup
ARMS = ("dh3", "dh7", "dh12", "iiwa14")
ALPHA = 0.01        # tests/tierb.py stat_tests' level
UNSUPPORTED, INVALID = ikpso._abi.IKPSO_ERR_UNSUPPORTED, ikpso._abi.IKPSO_ERR_INVALID_ARG
# FAST tolerance on a fitness (tests/tierb.py TOLS, rel_fitness) ...
REL = dict(tierb.TOLS)["rel_fitness"]
# ... plus an absolute floor for values near zero: four times the largest |gpu - float64| seen over
# every case of test_fitness_is_what_the_header_says on the first GPU run (1.476e-6, dh3 at P = 1024)
FLOOR = 4 * 1.476e-6


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Case:
    """An arm, its axis mask, its fitness configuration and B x T reachable pose targets."""

    def __init__(self, name, nb=B, frames=T, seed=11):
        self.name = name
        if name == "iiwa14":
            self.arm, self.fit = iiwa14(), ikpso.FitnessConfig(0.0, 0.0, 0.1)  # the dh7 workload's
        else:
            self.arm, self.fit = tp.dh_arm_n(int(name[2:]))[0], ikpso.MAIN_FITNESS
        self.chain, self.mask = self.arm.origin.to_cuda(), self.arm.axis_mask
        rng = np.random.default_rng([seed, len(self.chain)])
        self.theta = tp.random_poses(self.chain, nb * frames, rng, self.mask)
        p, R = pose64.poses(self.chain, self.theta, self.mask)
        self.targets = p.astype(np.float32).reshape(frames, nb, 1, 3)
        self.rot = R.astype(np.float32).reshape(frames, nb, 3, 3)

    def solver(self, P, iterations=IT, **kw):
        kw.setdefault("kernel", "resident")
        kw.setdefault("axis_mask", self.mask)
        return ikpso.BatchSolver(self.chain, P, pso=ikpso.PSOConfig(0.5, 0.5, 1.25, iterations), fit=self.fit, **kw)


@pytest.fixture(scope="module")
def cases(device):
    return {name: Case(name) for name in ARMS}


def run_track(case, P, stop=None, iterations=IT, frames=slice(None), **pose):
    """solve_track on a fresh solver: [angles, fitness, residual, iterations, states], kernel name.
    pose: weight=... runs the pose entry with the case's orientation targets."""
    s = case.solver(P, iterations)
    nb = case.targets.shape[1]
    s.seed(nb)
    kw = {}
    if "weight" in pose:
        kw = dict(target_rot=dev(case.rot[frames]), orientation_weight=pose["weight"])
    out = [t.cpu().numpy() for t in s.solve_track(dev(case.targets[frames]), iterations=iterations,
                                                  stop_fitness=stop, **kw)]
    out.append(s.generator_states(0, nb))
    name = s.kernel
    s.close()
    return out, name


def run_loop(case, P, stop, weight, iterations=IT):
    """The frame contract's checker: one frames = 1 pose call (solve_until) per frame on a fresh
    solver, each fed the previous answers.  Also the generator states after frame 0."""
    s = case.solver(P, iterations)
    nb = case.targets.shape[1]
    s.seed(nb)
    frames, prev, first_states = [[], [], [], []], None, None
    for t in range(case.targets.shape[0]):
        out = s.solve_until(dev(case.targets[t]), start_pose=prev, max_iterations=iterations,
                            stop_fitness=-1.0 if stop is None else stop, target_rot=dev(case.rot[t]),
                            orientation_weight=weight)
        prev = out[0]
        for acc, o in zip(frames, out):
            acc.append(o.cpu().numpy())
        if t == 0:
            first_states = s.generator_states(0, nb)
    out = [np.stack(f) for f in frames]
    out.append(s.generator_states(0, nb))
    s.close()
    return out, first_states


def assert_same(got, want, rows=None):
    for name, g, w in zip(("angles", "fitness", "residual", "iterations", "generator states"), got, want):
        if rows is not None:
            g, w = g[rows], w[rows]
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(bits(g), bits(w)), (name, np.argwhere(bits(g) != bits(w))[:8].tolist())


# ------------------------------------------------------------------ 1. weight zero is today's track
@pytest.mark.parametrize("stopping", [False, True], ids=["never-stops", "median-stop"])
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("name", ARMS)
def test_weight_zero_is_solve_track(cases, name, P, stopping):
    """Weight 0 is the term absent (the entry then runs the track kernel without it): bit for bit the
    call without target_rot -- angles, fitness, residual, iteration counts and generator states."""
    case = cases[name]
    plain, kname = run_track(case, P)
    assert f"swarm_resident<dh{case.arm.joints}>" in kname, kname
    stop = float(np.median(plain[1])) if stopping else None  # (from the checker: the call without target_rot)
    want = run_track(case, P, stop)[0] if stopping else plain
    got, _ = run_track(case, P, stop, weight=0.0)
    assert_same(got, want)
    if stopping:
        assert (want[3] < IT).any() and (want[3] == IT).any(), want[3].tolist()


# ------------------------------------------------------------ 2. the fitness is what the header says
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("name", ARMS)
def test_fitness_is_what_the_header_says(cases, name, P):
    case = cases[name]
    (ang, fit, res, its, _), _ = run_track(case, P, weight=1.0)
    assert (its == IT).all()
    D = ang.shape[2]
    start = np.array([case.chain["rotation"][k][c] for k, c in tp.free_axes(case.chain, case.mask)], np.float32)
    rest = np.concatenate([np.broadcast_to(start, (1, B, D)), ang[:-1]])  # frame t starts from frame t-1's answer
    want = pose64.pose_fitness(case.chain, case.mask, case.fit.angle_weight, ang.reshape(-1, D), rest.reshape(-1, D),
                               case.targets, case.rot, 1.0).reshape(T, B)
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


# -------------------------------------------------------------------------------- 3. the frame loop
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
                                                      target_rot=dev(case.rot[0]), orientation_weight=1.0)]
        states = s.generator_states(0, B).reshape(B, P, -1)
        s.close()
        rows = n[0] == count
        assert (out[3] == count).all()
        for k, label in enumerate(("angles", "fitness", "residual")):
            assert np.array_equal(bits(out[k][rows]), bits(want[k][0][rows])), (label, count)
        assert np.array_equal(states[rows], first_states.reshape(B, P, -1)[rows]), count


# ----------------------------------------------------------------- 4. it steers; 5. the tool frame
@pytest.fixture(scope="module")
def steering(device):
    """iiwa, 64 swarms x 1024 particles x 100 iterations, one frame, the same seeds: orientation
    weight 1 against weight 0.  The targets are given as textbook DH tool poses and handed over
    through DHArm.node_target."""
    nb, P, iters = 64, 1024, 100
    case = Case("iiwa14", nb=nb, frames=1, seed=12)
    arm = case.arm
    theta = np.array([arm.joint_angles(x) for x in case.theta])
    tool = np.array([dh_forward_pose(t, IIWA14["d"], IIWA14["a"], IIWA14["alpha"]) for t in theta])
    targets = tool[:, :3, 3].astype(np.float32).reshape(nb, 1, 3)
    r_tool = tool[:, :3, :3]
    node_rot = arm.node_target(r_tool).astype(np.float32)
    assert np.max(np.abs(targets - case.targets[0])) <= 1e-6 and np.max(np.abs(node_rot - case.rot[0])) <= 1e-6
    runs = {}
    for w in (1.0, 0.0):
        s = case.solver(P, iters)
        s.seed(nb)
        runs[w] = [t.cpu().numpy() for t in s.solve_until(dev(targets), max_iterations=iters, stop_fitness=-1.0,
                                                          target_rot=dev(node_rot), orientation_weight=w)]
        s.close()
    return case, node_rot, r_tool, runs


def sign_test_smaller(with_term, without):
    """tests/tierb.py's strict paired sign test (only exactly equal values tie), H0 "the term is as
    likely to leave the angle larger as smaller" against "smaller": (smaller, larger, p)."""
    from scipy.stats import binomtest

    smaller, larger = int(np.sum(with_term < without)), int(np.sum(with_term > without))
    assert tierb.SIGN_TIE == 0.0
    p = float(binomtest(smaller, smaller + larger, 0.5, alternative="greater").pvalue) if smaller + larger else 1.0
    return smaller, larger, p


def test_it_steers(steering):
    case, node_rot, _, runs = steering
    ang = {w: pose64.geodesic(pose64.poses(case.chain, runs[w][0], case.mask)[1], node_rot) for w in runs}
    smaller, larger, p = sign_test_smaller(ang[1.0], ang[0.0])
    print(f"geodesic angle to the target, median: weight 1 {np.median(ang[1.0]):.4e} rad, weight 0 "
          f"{np.median(ang[0.0]):.4e} rad; residual, median: weight 1 {np.median(runs[1.0][2]):.4e}, weight 0 "
          f"{np.median(runs[0.0][2]):.4e}; smaller in {smaller} of 64, larger in {larger}, p = {p:.3e}")
    assert len(ang[1.0]) == 64 and p < ALPHA, (smaller, larger, p)


def test_tool_frame(steering):
    case, _, r_tool, runs = steering
    ang = {}
    for w in runs:
        theta = np.array([case.arm.joint_angles(x) for x in runs[w][0]])
        got = np.array([dh_forward_pose(t, IIWA14["d"], IIWA14["a"], IIWA14["alpha"])[:3, :3] for t in theta])
        ang[w] = pose64.geodesic(got, r_tool)
    smaller, larger, p = sign_test_smaller(ang[1.0], ang[0.0])
    print(f"tool-frame angle, median: weight 1 {np.median(ang[1.0]):.4e} rad, weight 0 {np.median(ang[0.0]):.4e} rad; "
          f"smaller in {smaller} of 64, larger in {larger}, p = {p:.3e}")
    assert len(ang[1.0]) == 64 and p < ALPHA, (smaller, larger, p)


# ----------------------------------------------------------------------------------- 6. refusals
def pose_status(s, case, weight=1.0, rot=True, frames=1):
    """The C entry's status on device buffers of the right sizes (nothing is read back)."""
    nb = case.targets.shape[1]
    tg, tr = dev(case.targets[:max(frames, 1)]), dev(case.rot[:max(frames, 1)])
    ang = torch.empty((max(frames, 1), nb, s.dof), dtype=torch.float32, device="cuda")
    fit = torch.empty((max(frames, 1), nb), dtype=torch.float32, device="cuda")
    st = s._lib.ikpso_solve_track_pose(s._h, tg.data_ptr(), tr.data_ptr() if rot else None, float(weight), None, nb,
                                       frames, IT, -1.0, ang.data_ptr(), fit.data_ptr(), None, None, None)
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
    assert pose_status(s, case) == UNSUPPORTED
    if how != "unmasked":
        with pytest.raises(ikpso.IkpsoError) as e:
            s.solve_track(dev(case.targets), target_rot=dev(case.rot), orientation_weight=1.0)
        assert e.value.status == UNSUPPORTED
    s.close()


def test_invalid_arguments_and_empty_calls(cases):
    case = cases["iiwa14"]
    s = case.solver(128)
    s.seed(B)
    before = s.generator_states(0, B)
    assert pose_status(s, case, weight=-1.0) == INVALID
    assert pose_status(s, case, weight=float("nan")) == INVALID
    assert pose_status(s, case, weight=1.0, rot=False) == INVALID
    assert pose_status(s, case, weight=0.0, rot=False) == ikpso._abi.IKPSO_OK  # weight 0 reads no target_rot
    s.seed(B)
    assert pose_status(s, case, frames=0) == ikpso._abi.IKPSO_OK
    lib = s._lib
    assert lib.ikpso_solve_track_pose(s._h, None, None, 0.0, None, B, 0, IT, -1.0, None, None, None, None, None) == 0
    # frames > 0 needs targets and out_angles, even with no swarm to solve
    st = lib.ikpso_solve_track_pose(s._h, None, None, 0.0, None, 0, T, IT, -1.0, None, None, None, None, None)
    assert st == INVALID
    assert np.array_equal(s.generator_states(0, B), before)  # no device work: the generators did not move
    s.close()


# ------------------------------------------------------------------------------ 7. the C example
def test_pose_from_plain_c(device):
    exe = Path(__file__).resolve().parents[1] / "examples" / "_build" / "pose_c"
    if not exe.exists():
        pytest.fail(f"{exe} not built (__graft_entry__.build() builds examples/)")
    r = subprocess.run([str(exe), "32", "100", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "swarm_resident<dh7>" in r.stdout and "finite 1" in r.stdout, r.stdout
    rows = re.findall(r"frame (\d+): position error (\S+) m, angle error (\S+) rad \(weight 0: (\S+) m, (\S+) rad\)",
                      r.stdout)
    assert [int(x[0]) for x in rows] == [0, 1, 2, 3], r.stdout
    for _, _, angle, _, angle0 in rows:
        assert float(angle) < float(angle0), r.stdout
