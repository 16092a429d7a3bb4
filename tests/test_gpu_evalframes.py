"""ikpso_solver_evaluate_frames on the GPU (BatchSolver.evaluate_frames): the node rotations, the rotation
error per effector and the fitness with the rotation term, for given angle vectors.

Checkers: tests/frames64.py in float64 (node_frames, frames_fitness: the header's definitions in numpy),
ikpso.dh.dh_forward_pose for the DH arm's tool frame, ikpso_solver_evaluate (all weights 0), the CPU oracle's
contact decisions, and the solves whose fitness the entry restates.  Every tolerance on a value is four
times what a float32 restatement of the same numpy expression differs from float64 by, over the same
poses: the spread of a valid fp32 evaluation with a margin of 4 for another operation order -- the
construction of tests/test_gpu_frames.py's `floor` fixture, from which REL is taken too.
"""
import ctypes

import numpy as np
import pytest

import frames64
import ikpso
import pose64
import tierb
import topologies as tp
from ikpso.dh import IIWA14, dh_forward_pose, iiwa14

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 257                                # two workgroups of the evaluate kernels, the second holding one lane
NAMES = ("ref7", "serial6", "generic5", "generic1", "serial20", "iiwa14", "ref7coll")
ARITHS = ("fast", "reference")
REL = dict(tierb.TOLS)["rel_fitness"]  # FAST tolerance on a fitness (tests/test_gpu_frames.py, tests/tierb.py TOLS)
MIXED = (1.0, 0.0, 0.5)                # cycled over the effectors (tests/test_gpu_frames.py)
FMAX = np.float32(np.finfo(np.float32).max)
OK, INVALID = ikpso._abi.IKPSO_OK, ikpso._abi.IKPSO_ERR_INVALID_ARG


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def rot_error64(R, T, dtype=np.float64):
    """|R - T|_F^2 over the last two axes, in dtype."""
    return np.sum((np.asarray(R, dtype=dtype) - np.asarray(T, dtype=dtype)) ** 2, axis=(-2, -1), dtype=dtype)


class Case:
    """A chain, N in-bounds poses with rest poses, and position and rotation targets that are the
    effector frames of N other in-bounds poses; the float64 answers and the float32 restatement's spread."""

    def __init__(self, name, n=N, seed=41):
        self.name, self.fit, self.mask, self.arm, self.boxes = name, ikpso.MAIN_FITNESS, None, None, None
        if name.startswith("ref7"):
            self.chain = ikpso.reference_scene(reset=True).origin.to_cuda()
            if name == "ref7coll":  # the collider fixture's two boxes (tests/test_tierb_fixtures.py)
                self.boxes = ikpso.init_colliders(4)[[0, 3]]
        elif name == "iiwa14":
            self.arm = iiwa14()
            self.chain, self.mask = self.arm.origin.to_cuda(), self.arm.axis_mask
        else:
            J = int(name.lstrip("abcdefghijklmnopqrstuvwxyz"))
            self.chain = tp.serial(J) if name.startswith("serial") else tp.random_tree(J, 0)
        self.J, self.eff = len(self.chain) - 1, tp.effectors(self.chain)
        self.E = len(self.eff)
        rng = np.random.default_rng([seed, len(self.chain)])
        self.x, self.rest, other = (tp.random_poses(self.chain, n, rng, self.mask) for _ in range(3))
        self.full = tp.expand(self.chain, self.x, self.mask)
        p64, self.R64 = frames64.node_frames(self.chain, self.full)
        p32, R32 = frames64.node_frames(self.chain, self.full, dtype=np.float32)
        self.rot_spread = float(np.max(np.abs(R32.astype(np.float64) - self.R64)))
        self.pos_spread = float(np.max(np.abs(p32.astype(np.float64) - p64)))
        p, R = frames64.effector_frames(self.chain, other, self.mask)
        self.targets, self.trot = p.astype(np.float32), R.astype(np.float32)
        self.err64 = rot_error64(self.R64[:, self.eff - 1], self.trot)
        err32 = rot_error64(R32[:, self.eff - 1], self.trot, dtype=np.float32)
        self.err_spread = float(np.max(np.abs(err32.astype(np.float64) - self.err64)))
        self.mixed = np.array([MIXED[e % 3] for e in range(self.E)], np.float32)
        self.want = self.fitness64(self.mixed)
        self.spread = float(np.max(np.abs(self.fitness64(self.mixed, np.float32).astype(np.float64) - self.want)))

    def fitness64(self, weights, dtype=np.float64, trot=None):
        """The header's fitness without a collider term (tests/frames64.py)."""
        return frames64.frames_fitness(self.chain, self.fit.angle_weight, self.x, self.rest, self.targets,
                                       self.trot if trot is None else trot, weights, self.mask, dtype=dtype)

    def solver(self, arith, P=64, **kw):
        if self.mask is not None:
            kw.setdefault("axis_mask", self.mask)
            kw.setdefault("kernel", "resident")  # FAST: the folded solver
        return ikpso.BatchSolver(self.chain, P, fit=self.fit, arith=arith, colliders=self.boxes, **kw)


@pytest.fixture(scope="module")
def cases(device):
    return {name: Case(name) for name in NAMES}


@pytest.fixture(scope="module")
def floor(cases):
    """tests/test_gpu_frames.py's FLOOR: four times the largest |float32 numpy evaluation - float64| of the
    header's fitness over every case.  From the restatement alone (both sides are tests/frames64.py)."""
    spread = max(c.spread for c in cases.values())
    print(f"fp32 restatement of the fitness against float64, max over every case: {spread:.3e}; FLOOR = {4 * spread:.3e}")
    return 4.0 * spread


@pytest.fixture(scope="module")
def floors(cases):
    """The same construction for the rotations, the rotation error and the positions: one figure each, four
    times the largest |float32 numpy evaluation - float64| over every case's poses, as `floor` is one figure
    over every case.  The cases' own spreads are printed beside it."""
    out = {}
    for what in ("rot", "err", "pos"):
        per = {n: getattr(c, what + "_spread") for n, c in cases.items()}
        out[what] = 4.0 * max(per.values())
        print(f"fp32 restatement of {what} against float64: " + ", ".join(f"{n} {v:.3e}" for n, v in per.items()) +
              f"; tolerance {out[what]:.3e}")
    return out


@pytest.fixture(scope="module")
def runs(cases):
    """Every (case, arithmetic) once: the entry with the mixed weights, with garbage in the weight-0
    targets, with no weights, with the GPU's own rotations as targets, on one vector -- and evaluate()."""
    out = {}
    for name, case in cases.items():
        for arith in ARITHS:
            s = case.solver(arith)
            if case.arm is not None and arith == "fast":
                assert s.kernel == f"swarm_resident<dh{case.arm.joints}>", s.kernel  # folded; evaluated in Euler form
            x, tg, rest, trot = dev(case.x), dev(case.targets), dev(case.rest), dev(case.trot)
            r = {"mixed": s.evaluate_frames(x, tg, rest, trot, case.mixed)}
            garbage = case.trot.copy()
            garbage[:, case.mixed == 0] = 7.0
            r["garbage"] = s.evaluate_frames(x, tg, rest, dev(garbage), case.mixed)
            r["zero"] = s.evaluate_frames(x, tg, rest, trot, np.zeros(case.E, np.float32))
            r["null"] = s.evaluate_frames(x, tg, rest)
            own = r["mixed"][2][:, torch.from_numpy(case.eff - 1).cuda()].contiguous()
            r["own"] = s.evaluate_frames(x, tg, rest, own, case.mixed)
            r["one"] = s.evaluate_frames(x[:1], tg[:1], rest[:1], trot[:1], case.mixed)
            r["evaluate"] = s.evaluate(x, tg, rest)
            out[(name, arith)] = {k: [None if t is None else t.cpu().numpy() for t in v] for k, v in r.items()}
            s.close()
    return out


def params():
    return [(n, a) for n in NAMES for a in ARITHS]


# ------------------------------------------------------------------------------------- 1. rotations
@pytest.mark.parametrize("name,arith", params())
def test_rotations(cases, runs, floors, name, arith):
    """Measured on an MI355X (tolerance 2.067e-6, four times serial20's spread of 5.167e-7, the largest): worst
    |R_gpu - R_float64| 5.2e-7 REFERENCE, 1.36e-6 FAST (both serial20); worst |R R^T - 1| 1.04e-6 REFERENCE
    (serial20), 1.74e-6 FAST (iiwa14; serial20 1.52e-6).  Without the FAST builds' compensation of the hardware
    sin/cos amplitude bias serial20 had |R R^T - 1| = 4.1e-6."""
    case = cases[name]
    fit, pos, rot, err = runs[(name, arith)]["mixed"]
    assert rot.shape == (N, case.J, 3, 3) and pos.shape == (N, case.J, 3) and err.shape == (N, case.E)
    d = float(np.max(np.abs(rot.astype(np.float64) - case.R64)))
    eye = rot.astype(np.float64) @ np.swapaxes(rot.astype(np.float64), -1, -2) - np.eye(3)
    print(f"{name} {arith}: J={case.J} max |R_gpu - R_float64| = {d:.3e}, max |R R^T - 1| = {np.max(np.abs(eye)):.3e}, "
          f"tolerance {floors['rot']:.3e} (four times this case's own spread: {4 * case.rot_spread:.3e})")
    assert np.isfinite(rot).all()
    assert d <= floors["rot"]
    assert float(np.max(np.abs(eye))) <= floors["rot"]
    # one vector alone: the same lane arithmetic, the same bits
    for a, b in zip(runs[(name, arith)]["one"], (fit, pos, rot, err)):
        assert np.array_equal(bits(a), bits(b[:1]))


@pytest.mark.parametrize("arith", ARITHS)
def test_dh_tool_frame(cases, runs, floors, arith):
    """The DH arm: node rotation times the arm's constant tool rotation is the textbook tool frame."""
    case = cases["iiwa14"]
    rot = runs[("iiwa14", arith)]["mixed"][2][:, -1].astype(np.float64)
    tool = np.array([dh_forward_pose(case.arm.joint_angles(v), IIWA14["d"], IIWA14["a"], IIWA14["alpha"])[:3, :3]
                     for v in case.x])
    d = float(np.max(np.abs(rot @ case.arm.tool_rotation - tool)))
    print(f"iiwa14 {arith}: max |R_node K - R_tool| = {d:.3e}, tolerance {floors['rot']:.3e}")
    assert d <= floors["rot"]
    assert float(np.max(np.abs(case.arm.node_target(tool) - rot))) <= floors["rot"]


# -------------------------------------------------------------------------------- 2. rotation error
@pytest.mark.parametrize("name,arith", params())
def test_rotation_error(cases, runs, floors, name, arith):
    """Measured on an MI355X (tolerance 9.382e-6, four times serial20's spread of 2.345e-6, the largest): worst
    |gpu - float64| 3.59e-6 REFERENCE, 6.12e-6 FAST (both serial20; 1.42e-5 FAST without the bias compensation);
    at the GPU's own rotations the error is exactly 0 everywhere."""
    case = cases[name]
    err = runs[(name, arith)]["mixed"][3].astype(np.float64)
    d = float(np.max(np.abs(err - case.err64)))
    own = runs[(name, arith)]["own"][3]
    print(f"{name} {arith}: |R - T|^2 {case.err64.min():.3e}..{case.err64.max():.3e}, max |gpu - float64| = {d:.3e}, "
          f"at the GPU's own rotations max {own.max():.3e}, tolerance {floors['err']:.3e} (four times this case's "
          f"own spread: {4 * case.err_spread:.3e})")
    assert d <= floors["err"]
    assert (own >= 0.0).all() and float(own.max()) <= floors["err"]
    # the helper: the geodesic angle of the same pairs
    want = frames64.geodesic(case.R64[:, case.eff - 1], case.trot)
    got = ikpso.rotation_angle(err)
    big = (want > 0.1) & (want < np.pi - 0.1)  # (the arccos form loses digits at both ends; these are random pairs)
    assert big.any() and float(np.max(np.abs(got[big] - want[big]))) <= 1e-4


# ------------------------------------------------------------------------------------- 3. fitness
@pytest.mark.parametrize("name,arith", params())
def test_fitness(cases, runs, floor, floors, name, arith):
    case, r = cases[name], runs[(name, arith)]
    fit = r["mixed"][0]
    clear = r["evaluate"][0] != FMAX  # (no collider term in the float64 expression: section 5 has the contacts)
    assert clear.all() or case.boxes is not None
    want = case.want
    e = np.abs(fit.astype(np.float64) - want)[clear]
    print(f"{name} {arith}: fitness {want.min():.3e}..{want.max():.3e}, max |gpu - float64| = {e.max():.3e}, max relative "
          f"{np.max(e / want[clear]):.3e}, FLOOR {floor:.3e}")
    assert (e <= REL * want[clear] + floor).all(), (e.max(), np.argwhere(e > REL * want[clear] + floor)[:4].tolist())
    assert (fit[~clear] == FMAX).all()
    # a weight of 0 never reads that effector's target into the sum
    if (case.mixed == 0).any():
        assert np.array_equal(bits(r["garbage"][0]), bits(fit))
        assert np.array_equal(bits(r["garbage"][2]), bits(r["mixed"][2]))
    # all weights 0, or none: evaluate()
    efit, epos = r["evaluate"]
    for key in ("zero", "null"):
        zfit, zpos = r[key][0], r[key][1]
        dfit = np.abs(zfit.astype(np.float64) - efit.astype(np.float64))[clear]
        dpos = np.abs(zpos.astype(np.float64) - epos.astype(np.float64))
        print(f"{name} {arith} weights {key}: max |fitness - evaluate's| = {dfit.max():.3e}, positions {dpos.max():.3e}")
        if arith == "reference":
            assert np.array_equal(bits(zfit), bits(efit)) and np.array_equal(bits(zpos), bits(epos))
        else:
            assert (dfit <= floor).all() and (zfit[~clear] == FMAX).all()
            assert float(dpos.max()) <= floors["pos"]
    assert r["null"][3] is None and r["zero"][3] is not None


# ------------------------------------------------------------------- 4. it agrees with the solvers
B, T, P, IT = 8, 2, 65, 20


def start_and_previous(case, ang):
    """rest of every (frame, swarm): the chain's rotations for frame 0, then the frame before's answer."""
    start = np.array([case.chain["rotation"][k][c] for k, c in tp.free_axes(case.chain, case.mask)], np.float32)
    return np.concatenate([np.broadcast_to(start, (1,) + ang.shape[1:]), ang[:-1]])


def test_agrees_with_solve_track_frames(cases, floor):
    case = cases["ref7"]
    tg, trot = case.targets[:T * B].reshape(T, B, case.E, 3), case.trot[:T * B].reshape(T, B, case.E, 3, 3)
    s = ikpso.BatchSolver(case.chain, P, pso=ikpso.PSOConfig(0.5, 0.5, 1.25, IT), fit=case.fit, kernel="resident")
    s.seed(B)
    ang, fit, _, _ = (t.cpu().numpy() for t in s.solve_track(dev(tg), iterations=IT, effector_rot=dev(trot),
                                                              effector_rot_weight=case.mixed))
    assert s.kernel.startswith("swarm_resident_frames<"), s.kernel
    D = ang.shape[2]
    got = s.evaluate_frames(dev(ang.reshape(-1, D)), dev(tg.reshape(-1, case.E, 3)),
                            dev(start_and_previous(case, ang).reshape(-1, D)), dev(trot.reshape(-1, case.E, 3, 3)),
                            case.mixed)[0].cpu().numpy().reshape(T, B)
    s.close()
    want = fit.astype(np.float64)
    e = np.abs(got.astype(np.float64) - want)
    print(f"ref7: solve fitness {want.min():.3e}..{want.max():.3e}, max |evaluate_frames - solve| = {e.max():.3e}, "
          f"max relative {np.max(e / want):.3e}, FLOOR {floor:.3e}")
    assert (e <= REL * want + floor).all(), e.max()


def test_agrees_with_solve_track_pose(cases, floor):
    """The folded arm's pose kernels against the Euler form: E = 1, orientation_weight = rot_weights[0]."""
    case, w = cases["iiwa14"], 0.5
    tg, trot = case.targets[:T * B].reshape(T, B, 1, 3), case.trot[:T * B].reshape(T, B, 3, 3)
    s = case.solver("fast", P, pso=ikpso.PSOConfig(0.5, 0.5, 1.25, IT))
    s.seed(B)
    ang, fit, _, _ = (t.cpu().numpy() for t in s.solve_track(dev(tg), iterations=IT, target_rot=dev(trot),
                                                              orientation_weight=w))
    assert s.kernel == f"swarm_resident<dh{case.arm.joints}>", s.kernel
    D = ang.shape[2]
    got = s.evaluate_frames(dev(ang.reshape(-1, D)), dev(tg.reshape(-1, 1, 3)),
                            dev(start_and_previous(case, ang).reshape(-1, D)), dev(trot.reshape(-1, 1, 3, 3)),
                            [w])[0].cpu().numpy().reshape(T, B)
    s.close()
    want = fit.astype(np.float64)
    e = np.abs(got.astype(np.float64) - want)
    print(f"iiwa14: solve fitness {want.min():.3e}..{want.max():.3e}, max |evaluate_frames - solve| = {e.max():.3e}, "
          f"max relative {np.max(e / want):.3e}, FLOOR {floor:.3e}")
    assert (e <= REL * want + floor).all(), e.max()
    # and both are the header's expression (tests/pose64.py)
    h = pose64.pose_fitness(case.chain, case.mask, case.fit.angle_weight, ang.reshape(-1, D),
                            start_and_previous(case, ang).reshape(-1, D), tg, trot, w).reshape(T, B)
    assert (np.abs(got - h) <= REL * h + floor).all()


# ------------------------------------------------------------------------------------ 5. colliders
@pytest.mark.parametrize("arith", ARITHS)
def test_colliders(cases, runs, oracle, floor, arith):
    case, r = cases["ref7coll"], runs[("ref7coll", arith)]
    hit = r["evaluate"][0] == FMAX
    ohit = np.array([oracle.fitness(case.chain, v, colliders=case.boxes) for v in case.x], dtype=np.float32) == FMAX
    print(f"ref7coll {arith}: {int(hit.sum())} of {N} poses touch a box (oracle: {int(ohit.sum())})")
    assert 0 < ohit.sum() < N and 0 < hit.sum() < N  # both outcomes
    if arith == "reference":
        assert np.array_equal(hit, ohit)
    else:
        assert np.mean(hit == ohit) >= 0.99  # (tests/test_gpu_collide.py: FAST tests separating axes, the reference GJK)
    for key in ("mixed", "zero", "null", "garbage"):
        fit = r[key][0]
        assert np.array_equal(fit == FMAX, hit), key  # with and without weights
    # clear of the boxes: the finite sum, which the weights raise by the float64 term
    added = case.want - case.fitness64(np.zeros(case.E))
    got = r["mixed"][0].astype(np.float64) - r["zero"][0].astype(np.float64)
    assert (added[~hit] > 0).all()
    assert (np.abs(got - added)[~hit] <= REL * case.want[~hit] + floor).all()
    # the rotations and the rotation error are reported for a pose in a box too
    assert np.isfinite(r["mixed"][2]).all() and np.isfinite(r["mixed"][3]).all()


# --------------------------------------------------------------------------------- 6. grid stride
def test_grid_stride(cases):
    """More vectors than the grid cap's 8192 x 256 lanes: the last one is a second trip of lane 0."""
    case = cases["generic1"]
    n = 8192 * 256 + 1
    rng = np.random.default_rng(43)
    lo, hi = case.chain["min_rotation"][1].astype(np.float64), case.chain["max_rotation"][1].astype(np.float64)
    x = (lo + rng.uniform(0.0, 1.0, (n, 3)) * (hi - lo)).astype(np.float32)
    x = np.clip(x, lo.astype(np.float32), hi.astype(np.float32))
    pick = np.concatenate([rng.choice(n - 1, 1000, replace=False), [n - 1]])
    trot = dev(case.trot[np.arange(n) % N])  # [n, 1, 3, 3]: the case's N targets over and over
    s = case.solver("fast")
    fit = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    err = torch.full((n, 1), -1.0, dtype=torch.float32, device="cuda")
    xs = dev(x)
    w = (ctypes.c_float * 1)(1.0)
    st = s._lib.ikpso_solver_evaluate_frames(s._h, xs.data_ptr(), None, None, trot.data_ptr(), w, n, fit.data_ptr(),
                                             None, None, err.data_ptr(), None)
    assert st == OK
    torch.cuda.synchronize()
    s.close()
    assert bool((fit >= 0).all()) and bool((err >= 0).all())  # every vector was written
    fit, err = fit[torch.from_numpy(pick).cuda()].cpu().numpy(), err[torch.from_numpy(pick).cuda(), 0].cpu().numpy()
    xp, tp_rot = x[pick], case.trot[pick % N]
    rest = np.broadcast_to(np.asarray(case.chain["rotation"][1], np.float32), xp.shape)
    tg = np.broadcast_to(case.chain["target_position"][case.eff].astype(np.float32), (len(pick), 1, 3))
    want, want32 = (frames64.frames_fitness(case.chain, case.fit.angle_weight, xp, rest, tg, tp_rot, [1.0], dtype=t)
                    for t in (np.float64, np.float32))
    _, R = frames64.effector_frames(case.chain, xp)
    _, R32 = frames64.effector_frames(case.chain, xp, dtype=np.float32)
    e64, e32 = rot_error64(R, tp_rot)[:, 0], rot_error64(R32, tp_rot, dtype=np.float32)[:, 0]
    ffloor = 4.0 * float(np.max(np.abs(want32.astype(np.float64) - want)))
    efloor = 4.0 * float(np.max(np.abs(e32.astype(np.float64) - e64)))
    df, de = np.abs(fit - want), np.abs(err - e64)
    print(f"n = {n}: max |fitness - float64| = {df.max():.3e} (last {df[-1]:.3e}; floor {ffloor:.3e}), "
          f"max |rot_error - float64| = {de.max():.3e} (last {de[-1]:.3e}; floor {efloor:.3e})")
    assert (df <= REL * want + ffloor).all() and (de <= efloor).all()


# --------------------------------------------------------------------------------------- 7. refusals
def test_refusals_and_the_empty_call(cases):
    case = cases["ref7"]
    s = case.solver("fast")
    n, E, J = 4, case.E, case.J
    x, trot = dev(case.x[:n]), dev(case.trot[:n])
    sentinel = -12345.0
    outs = [torch.full(shape, sentinel, dtype=torch.float32, device="cuda")
            for shape in ((n,), (n, J, 3), (n, J, 9), (n, E))]

    def call(weights, rot=True, err=True, count=n):
        w = None if weights is None else (ctypes.c_float * E)(*weights)
        st = s._lib.ikpso_solver_evaluate_frames(s._h, x.data_ptr(), None, None, trot.data_ptr() if rot else None, w,
                                                 count, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                                 outs[3].data_ptr() if err else None, None)
        torch.cuda.synchronize()
        return st

    for bad in (-1.0, float("nan"), float("inf")):
        assert call((1.0, bad, 0.0)) == INVALID, bad
        assert call((0.0, 0.0, bad), rot=False, err=False) == INVALID, bad
    assert call((0.0, 0.5, 0.0), rot=False, err=False) == INVALID  # a weight > 0 needs target_rot
    assert call(None, rot=False, err=True) == INVALID              # so does out_rot_error
    assert call((0.0, 0.0, 0.0), rot=False, err=True) == INVALID
    assert call((1.0, 1.0, 1.0), count=-1) == INVALID
    assert call((1.0, 1.0, 1.0), count=0) == OK                    # no device work ...
    assert s._lib.ikpso_solver_evaluate_frames(s._h, None, None, None, None, None, 0, None, None, None, None, None) == OK
    for o in outs:
        assert bool((o == sentinel).all())                         # ... and nothing refused wrote anything
    assert call((0.0, 0.0, 0.0), rot=False, err=False) == OK       # all weights 0 reads no target_rot
    assert call(None, rot=False, err=False) == OK
    assert bool((outs[0] != sentinel).all()) and bool((outs[2] != sentinel).all()) and bool((outs[3] == sentinel).all())
    assert s._lib.ikpso_solver_evaluate_frames(s._h, None, None, None, None, None, n, None, None, None, None, None) == INVALID
    s.close()
