"""Orientation targets per effector on the GPU: BatchSolver.solve_track / solve_until with effector_rot
(ikpso_solve_track_frames), the Euler topologies' track kernels with a rotation term per effector.

The oracle has no orientation term, so the checkers are: the existing solve_track (all weights 0 must
equal it bit for bit), a loop of one-frame calls (the frame contract), the fitness recomputed in numpy
float64 from the node table and the header's definition (tests/frames64.py), and for "does it steer"
the weight-0 run itself -- the parent's behaviour -- under tests/tierb.py's strict paired sign test.

Targets are the float64 effector frames of random in-bounds joint vectors, so every one is reachable.
"""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import frames64
import ikpso
import tierb
import topologies as tp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, T, IT = 8, 3, 30
NAMES = ("ref7", "serial6", "serial20", "generic1", "generic3", "generic20")
ALPHA = 0.01  # tests/tierb.py stat_tests' level
OK, UNSUPPORTED, INVALID = ikpso._abi.IKPSO_OK, ikpso._abi.IKPSO_ERR_UNSUPPORTED, ikpso._abi.IKPSO_ERR_INVALID_ARG
REL = dict(tierb.TOLS)["rel_fitness"]  # FAST tolerance on a fitness (tests/tierb.py TOLS)
MIXED = (1.0, 0.0, 0.5)                # cycled over the effectors


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def make_chain(name):
    if name == "ref7":
        return ikpso.reference_scene(reset=True).origin.to_cuda()
    J = int(name.lstrip("abcdefghijklmnopqrstuvwxyz"))
    return tp.serial(J) if name.startswith("serial") else tp.random_tree(J, 0)


class Case:
    """A chain and nb x frames reachable effector frames: targets [T, B, E, 3], rot [T, B, E, 3, 3]."""

    def __init__(self, name, nb=B, frames=T, seed=21):
        self.name, self.chain, self.fit = name, make_chain(name), ikpso.MAIN_FITNESS
        self.E = len(tp.effectors(self.chain))
        self.sizes = (65, tp.full_workgroup(3 * (len(self.chain) - 1)))  # a second wave with one lane; the largest
        rng = np.random.default_rng([seed, len(self.chain)])
        self.theta = tp.random_poses(self.chain, nb * frames, rng)
        p, R = frames64.effector_frames(self.chain, self.theta)
        self.targets = p.astype(np.float32).reshape(frames, nb, self.E, 3)
        self.rot = R.astype(np.float32).reshape(frames, nb, self.E, 3, 3)
        self.mixed = np.array([MIXED[e % 3] for e in range(self.E)], np.float32)

    def solver(self, P, iterations=IT, **kw):
        kw.setdefault("kernel", "resident")
        return ikpso.BatchSolver(self.chain, P, pso=ikpso.PSOConfig(0.5, 0.5, 1.25, iterations), fit=self.fit, **kw)


@pytest.fixture(scope="module")
def cases(device):
    return {name: Case(name) for name in NAMES}


def case_sizes():
    return [(n, which) for n in NAMES for which in (0, 1)]


def size_id(v):
    return v if isinstance(v, str) else ("small", "full")[v]


def run_track(case, P, stop=None, iterations=IT, frames=slice(None), **term):
    """solve_track on a fresh solver: [angles, fitness, residual, iterations, states], kernel name.
    term: weights=... runs the frames entry with the case's rotation targets (rot=False: none given)."""
    s = case.solver(P, iterations)
    nb = case.targets.shape[1]
    s.seed(nb)
    kw = {}
    if "weights" in term:
        kw = dict(effector_rot=dev(case.rot[frames]) if term.get("rot", True) else None,
                  effector_rot_weight=term["weights"])
    out = [t.cpu().numpy() for t in s.solve_track(dev(case.targets[frames]), iterations=iterations,
                                                  stop_fitness=stop, **kw)]
    out.append(s.generator_states(0, nb))
    name = s.kernel
    s.close()
    return out, name


def run_loop(case, P, stop, weights, iterations=IT):
    """The frame contract's checker: one frames = 1 call (solve_until) per frame on a fresh solver, each
    fed the previous answers.  Also the generator states after frame 0."""
    s = case.solver(P, iterations)
    nb = case.targets.shape[1]
    s.seed(nb)
    frames, prev, first_states = [[], [], [], []], None, None
    for t in range(case.targets.shape[0]):
        out = s.solve_until(dev(case.targets[t]), start_pose=prev, max_iterations=iterations,
                            stop_fitness=-1.0 if stop is None else stop, effector_rot=dev(case.rot[t]),
                            effector_rot_weight=weights)
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


# ---------------------------------------------------------------- 1. all weights zero is today's track
@pytest.mark.parametrize("stopping", [False, True], ids=["never-stops", "median-stop"])
@pytest.mark.parametrize("name,which", case_sizes(), ids=size_id)
def test_weights_zero_is_solve_track(cases, name, which, stopping):
    """All weights 0, and no weights at all, are the term absent (the entry then runs the track kernel
    without it): bit for bit the call without effector_rot -- angles, fitness, residual, iteration counts
    and generator states -- and the kernel reported is the plain track kernel's."""
    case = cases[name]
    P = case.sizes[which]
    plain, kname = run_track(case, P)
    assert kname.startswith("swarm_resident<") and "frames" not in kname, kname
    stop = float(np.median(plain[1])) if stopping else None  # (from the checker: the call without the term)
    want = run_track(case, P, stop)[0] if stopping else plain
    got, gname = run_track(case, P, stop, weights=np.zeros(case.E, np.float32), rot=False)  # (no target_rot either)
    assert_same(got, want)
    assert gname == kname, (gname, kname)
    got, gname = run_track(case, P, stop, weights=None)  # rot_weights NULL
    assert_same(got, want)
    assert gname == kname, (gname, kname)
    if stopping:
        assert (want[3] < IT).any() and (want[3] == IT).any(), want[3].tolist()


def test_null_weights_through_the_c_entry(cases):
    """rot_weights NULL with a target_rot given: all weights 0 again."""
    case = cases["generic3"]
    want, _ = run_track(case, 65)
    s = case.solver(65)
    s.seed(B)
    ang = torch.empty((T, B, s.dof), dtype=torch.float32, device="cuda")
    fit = torch.empty((T, B), dtype=torch.float32, device="cuda")
    tg, tr = dev(case.targets), dev(case.rot)
    st = s._lib.ikpso_solve_track_frames(s._h, tg.data_ptr(), tr.data_ptr(), None, None, B, T, IT, -1.0,
                                         ang.data_ptr(), fit.data_ptr(), None, None, None)
    assert st == OK
    torch.cuda.synchronize()
    assert np.array_equal(bits(ang.cpu().numpy()), bits(want[0])) and np.array_equal(bits(fit.cpu().numpy()), bits(want[1]))
    assert np.array_equal(s.generator_states(0, B), want[4])
    s.close()


# ------------------------------------------------------------ 2. the fitness is what the header says
def header_fitness(case, ang, weights, dtype=np.float64):
    D = ang.shape[2]
    start = np.asarray(case.chain["rotation"][1:], np.float32).reshape(-1)
    rest = np.concatenate([np.broadcast_to(start, (1, B, D)), ang[:-1]])  # frame t starts from frame t-1's answer
    return frames64.frames_fitness(case.chain, case.fit.angle_weight, ang.reshape(-1, D), rest.reshape(-1, D),
                                   case.targets, case.rot, weights, dtype=dtype).reshape(T, B)


@pytest.fixture(scope="module")
def mixed_runs(cases):
    """Every case at both sizes with the mixed weights, never stopping: the GPU's outputs."""
    return {(n, w): run_track(cases[n], cases[n].sizes[w], weights=cases[n].mixed) for n, w in case_sizes()}


@pytest.fixture(scope="module")
def floor(cases, mixed_runs):
    """Four times the largest |float32 numpy evaluation - float64| of the header's expression over the
    answers of every case: the spread of a valid fp32 evaluation, with a margin of 4 for another
    operation order.  From the restatement alone (both sides are tests/frames64.py)."""
    spread = 0.0
    for (n, w), (out, _) in mixed_runs.items():
        f64 = header_fitness(cases[n], out[0], cases[n].mixed)
        f32 = header_fitness(cases[n], out[0], cases[n].mixed, dtype=np.float32)
        spread = max(spread, float(np.max(np.abs(f32.astype(np.float64) - f64))))
    print(f"fp32 restatement against float64, max over every case: {spread:.3e}; FLOOR = {4 * spread:.3e}")
    return 4.0 * spread


@pytest.mark.parametrize("name,which", case_sizes(), ids=size_id)
def test_fitness_is_what_the_header_says(cases, mixed_runs, floor, name, which):
    case = cases[name]
    (ang, fit, res, its, _), kname = mixed_runs[(name, which)]
    assert kname.startswith("swarm_resident_frames<"), kname
    assert (its == IT).all()
    D = ang.shape[2]
    want = header_fitness(case, ang, case.mixed)
    err = np.abs(fit.astype(np.float64) - want)
    print(f"{name} P={case.sizes[which]} E={case.E}: fitness {want.min():.3e}..{want.max():.3e}, max |gpu - float64| = "
          f"{err.max():.3e}, max relative {np.max(err / want):.3e}, FLOOR {floor:.3e}")
    assert np.isfinite(fit).all()
    assert (err <= REL * want + floor).all(), (err.max(), np.argwhere(err > REL * want + floor)[:4].tolist())
    # the residual stays the positional checkDistance residual
    p, _ = frames64.effector_frames(case.chain, ang.reshape(-1, D))
    want_res = np.linalg.norm(p - case.targets.reshape(-1, case.E, 3).astype(np.float64), axis=2).sum(axis=1)
    assert np.max(np.abs(res - want_res.reshape(T, B))) <= 1e-4, np.max(np.abs(res - want_res.reshape(T, B)))
    # an effector of weight 0 contributes nothing: the float64 fitness without it matches too
    if (case.mixed == 0).any():
        garbage = case.rot.copy()
        garbage[:, :, case.mixed == 0] = 7.0
        D = ang.shape[2]
        start = np.asarray(case.chain["rotation"][1:], np.float32).reshape(-1)
        rest = np.concatenate([np.broadcast_to(start, (1, B, D)), ang[:-1]])
        without = frames64.frames_fitness(case.chain, case.fit.angle_weight, ang.reshape(-1, D), rest.reshape(-1, D),
                                          case.targets, garbage, case.mixed).reshape(T, B)
        assert np.array_equal(without, want)


# -------------------------------------------------------------------------------- 3. the frame loop
@pytest.mark.parametrize("name,which", case_sizes(), ids=size_id)
def test_frame_loop(cases, name, which):
    case = cases[name]
    P, w = case.sizes[which], case.mixed if case.E > 1 else np.ones(1, np.float32)
    # the threshold as tests/test_gpu_track.py's median_threshold takes it: the median fitness of a
    # never-stopping checker loop
    stop = float(np.median(run_loop(case, P, None, w)[0][1]))
    want, first_states = run_loop(case, P, stop, w)
    got, _ = run_track(case, P, stop, weights=w)
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
                                                      effector_rot=dev(case.rot[0]), effector_rot_weight=w)]
        states = s.generator_states(0, B).reshape(B, P, -1)
        s.close()
        rows = n[0] == count
        assert (out[3] == count).all()
        for k, label in enumerate(("angles", "fitness", "residual")):
            assert np.array_equal(bits(out[k][rows]), bits(want[k][0][rows])), (label, count)
        assert np.array_equal(states[rows], first_states.reshape(B, P, -1)[rows]), count


# ------------------------------------------------------------------------------------- 4. it steers
def sign_test_smaller(with_term, without):
    """tests/tierb.py's strict paired sign test (only exactly equal values tie), H0 "the term is as
    likely to leave the angle larger as smaller" against "smaller": (smaller, larger, p)."""
    from scipy.stats import binomtest

    smaller, larger = int(np.sum(with_term < without)), int(np.sum(with_term > without))
    assert tierb.SIGN_TIE == 0.0
    p = float(binomtest(smaller, smaller + larger, 0.5, alternative="greater").pvalue) if smaller + larger else 1.0
    return smaller, larger, p


def test_it_steers(device):
    """The reference tree, 64 swarms x 1024 particles x 100 iterations, one frame, the same seeds: weight
    1 on every effector against weight 0, the parent's behaviour."""
    nb, P, iters = 64, 1024, 100
    case = Case("ref7", nb=nb, frames=1, seed=22)
    runs = {}
    for w in (1.0, 0.0):
        s = case.solver(P, iters)
        s.seed(nb)
        runs[w] = [t.cpu().numpy() for t in s.solve_until(dev(case.targets[0]), max_iterations=iters, stop_fitness=-1.0,
                                                          effector_rot=dev(case.rot[0]), effector_rot_weight=w)]
        s.close()
    ang = {w: frames64.geodesic(frames64.effector_frames(case.chain, runs[w][0])[1], case.rot[0]) for w in runs}
    for e in range(case.E):
        smaller, larger, p = sign_test_smaller(ang[1.0][:, e], ang[0.0][:, e])
        print(f"effector {e}: geodesic angle to the target, median: weight 1 {np.median(ang[1.0][:, e]):.4e} rad, "
              f"weight 0 {np.median(ang[0.0][:, e]):.4e} rad; smaller in {smaller} of {nb}, larger in {larger}, "
              f"p = {p:.3e}")
        assert len(ang[1.0]) == 64 and p < ALPHA, (e, smaller, larger, p)
    print(f"residual, median: weight 1 {np.median(runs[1.0][2]):.4e}, weight 0 {np.median(runs[0.0][2]):.4e}")


# ----------------------------------------------------------------------------------- 5. refusals
def frames_status(s, case, weights="ones", rot=True, frames=1, nb=None):
    """The C entry's status on device buffers of the right sizes (nothing is read back)."""
    import ctypes

    nb = case.targets.shape[1] if nb is None else nb
    n = max(frames, 1)
    E = s.effectors
    tg = torch.zeros((n, max(nb, 1), E, 3), dtype=torch.float32, device="cuda")
    tr = torch.zeros((n, max(nb, 1), E, 3, 3), dtype=torch.float32, device="cuda")
    ang = torch.empty((n, max(nb, 1), s.dof), dtype=torch.float32, device="cuda")
    fit = torch.empty((n, max(nb, 1)), dtype=torch.float32, device="cuda")
    w = None if weights is None else (ctypes.c_float * E)(*([1.0] * E if isinstance(weights, str) else list(weights)))
    st = s._lib.ikpso_solve_track_frames(s._h, tg.data_ptr(), tr.data_ptr() if rot else None, w, None, nb, frames, IT,
                                         -1.0, ang.data_ptr(), fit.data_ptr(), None, None, None)
    torch.cuda.synchronize()
    return st


def refused_solver(how):
    ref = ikpso.reference_scene(reset=True).origin.to_cuda()
    pso = ikpso.PSOConfig(0.5, 0.5, 1.25, IT)
    if how == "reference":
        return ikpso.BatchSolver(ref, 128, pso=pso, arith="reference", kernel="resident")
    if how in ("folded", "nofold"):
        arm = tp.dh_arm_n(7)[0]
        return ikpso.BatchSolver(arm.origin.to_cuda(), 128, pso=pso, kernel="resident", axis_mask=arm.axis_mask,
                                 fold=how == "folded")
    if how == "collider":  # a box the arm reaches: the collider term is live
        box = ikpso.make_collider((0.6, 0.6, 0.6), (0.0, 0.9, -1.6))
        return ikpso.BatchSolver(ref, 128, pso=pso, kernel="resident", colliders=box)
    if how == "auto":  # a swarm above one workgroup: AUTO picks another family
        return ikpso.BatchSolver(ref, 4096, pso=pso)
    return ikpso.BatchSolver(ref, 4096 if how == "coop" else 128, pso=pso, kernel=how)


@pytest.mark.parametrize("how", ["reference", "folded", "nofold", "collider", "streaming", "coop", "auto"])
def test_unsupported_solvers(cases, how):
    s = refused_solver(how)
    if how == "collider":
        assert s.collider_count > 0
    if how == "auto":
        assert "swarm_resident" not in s.kernel, s.kernel
    s.seed(B)
    before = s.generator_states(0, B)
    E = s.effectors
    assert frames_status(s, cases["ref7"]) == UNSUPPORTED
    assert frames_status(s, cases["ref7"], frames=0) == UNSUPPORTED  # before the empty call's return
    assert frames_status(s, cases["ref7"], weights=None, rot=False) == UNSUPPORTED  # no weight-0 detour either
    tg = torch.zeros((T, B, E, 3), dtype=torch.float32, device="cuda")
    tr = torch.zeros((T, B, E, 3, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(ikpso.IkpsoError) as e:
        s.solve_track(tg, effector_rot=tr, effector_rot_weight=1.0)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ikpso.IkpsoError) as e:
        s.solve_until(tg[0], effector_rot=tr[0], effector_rot_weight=1.0)
    assert e.value.status == UNSUPPORTED
    assert np.array_equal(s.generator_states(0, B), before)
    s.close()


def test_pose_and_aim_still_refuse_unmasked_chains(cases):
    """The folded-arm entries keep their refusals, and the three forms are not combined."""
    case = cases["serial6"]
    s = case.solver(128)
    s.seed(B)
    tg, tr = dev(case.targets), dev(case.rot)
    with pytest.raises(ikpso.IkpsoError) as e:
        s.solve_track(tg, target_rot=tr[:, :, 0].contiguous(), orientation_weight=1.0)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ikpso.IkpsoError) as e:
        s.solve_track(tg, aim_dir=tr[:, :, 0, 0].contiguous(), aim_weight=1.0)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(ValueError):
        s.solve_track(tg, effector_rot=tr, effector_rot_weight=1.0, target_rot=tr[:, :, 0].contiguous(), orientation_weight=1.0)
    with pytest.raises(ValueError):
        s.solve_until(tg[0], effector_rot=tr[0], effector_rot_weight=1.0, aim_dir=tr[0, :, 0, 0].contiguous(), aim_weight=1.0)
    with pytest.raises(ValueError):
        s.solve_track(tg, effector_rot=tr, effector_rot_weight=[1.0, 2.0])  # one weight, or E of them
    s.close()


# ------------------------------------------------------------- 6. invalid arguments and empty calls
def test_invalid_arguments_and_empty_calls(cases):
    case = cases["ref7"]
    s = case.solver(128)
    s.seed(B)
    before = s.generator_states(0, B)
    for bad in (-1.0, float("nan"), float("inf")):
        assert frames_status(s, case, weights=(1.0, bad, 0.0)) == INVALID, bad
        assert frames_status(s, case, weights=(0.0, 0.0, bad), rot=False) == INVALID, bad
    assert frames_status(s, case, weights=(0.0, 0.5, 0.0), rot=False) == INVALID  # a weight > 0 needs target_rot
    lib = s._lib
    nan = float("nan")
    assert lib.ikpso_solve_track_frames(s._h, None, None, None, None, B, 0, IT, nan, None, None, None, None, None) == INVALID
    # frames > 0 needs targets and out_angles, even with no swarm to solve
    assert lib.ikpso_solve_track_frames(s._h, None, None, None, None, 0, T, IT, -1.0, None, None, None, None, None) == INVALID
    # empty calls: OK, no device work
    assert frames_status(s, case, frames=0) == OK
    assert frames_status(s, case, nb=0) == OK
    assert lib.ikpso_solve_track_frames(s._h, None, None, None, None, B, 0, IT, -1.0, None, None, None, None, None) == OK
    assert np.array_equal(s.generator_states(0, B), before)  # no device work: the generators did not move
    # all weights 0 reads no target_rot
    assert frames_status(s, case, weights=(0.0, 0.0, 0.0), rot=False) == OK
    s.close()


# ------------------------------------------------------------------------------ 7. the C example
def test_frames_from_plain_c(device):
    exe = Path(__file__).resolve().parents[1] / "examples" / "_build" / "frames_c"
    if not exe.exists():
        pytest.fail(f"{exe} not built (__graft_entry__.build() builds examples/)")
    r = subprocess.run([str(exe), "32", "100"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert "kernel swarm_resident_frames<ref_tree7> (weights 0: swarm_resident<ref_tree7>)" in r.stdout, r.stdout
    assert "finite 1" in r.stdout, r.stdout
    rows = re.findall(r"effector (\d+): angle error (\S+) rad \(weights 0: (\S+) rad\)", r.stdout)
    assert [int(x[0]) for x in rows] == [0, 1, 2], r.stdout
    for _, angle, angle0 in rows:
        assert float(angle) < float(angle0), r.stdout
