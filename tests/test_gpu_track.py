"""BatchSolver.solve_track (ikpso_solve_track) on the GPU: B swarms following T waypoints each,
every frame warm-started from the previous frame's answer, in one launch on the resident family.

The statement under test is exact, and its checker is the loop of calls that already exist: a
second solver, seeded identically, runs solve_until(targets[t], start_pose=previous angles) for
t = 0..T-1.  Angles, fitness, residual, iteration counts and the generator states left in the
solver are compared on bit patterns, in FAST arithmetic as in REFERENCE.

Targets: the first 16 swarms follow reachable paths (the effector positions evaluate() returns for
angle vectors interpolated between two random in-bounds poses; frame 3 repeats frame 2's targets),
the last 8 have targets at ten times the arm's reach.  A threshold never comes from the code under
test: it is the median fitness of the reachable cells of a non-stopping checker loop.
"""
import numpy as np
import pytest

import ikpso

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, REACHABLE, T, IT = 24, 16, 6, 12
PSO = ikpso.PSOConfig(0.5, 0.5, 1.25, IT)
PATH_POS = np.array([0, 1, 2, 2, 3, 4], dtype=np.float64)  # frame 3 repeats frame 2
# the early-stop conditions (test_early_stop) hold for this seed and step on the checker
SEED, STEP = 2024, 0.02


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def path_targets(chain, mask=None, seed=SEED, step=STEP, frames=T):
    """[frames, 24, E, 3] float32 targets (module docstring) of a chain with an optional axis mask."""
    rng = np.random.default_rng(seed)
    free = [(k, c) for k in range(1, len(chain)) for c in range(3) if mask is None or (int(mask[k]) >> c) & 1]
    lo = np.array([chain["min_rotation"][k][c] for k, c in free], dtype=np.float64)
    hi = np.array([chain["max_rotation"][k][c] for k, c in free], dtype=np.float64)
    a0 = lo + rng.uniform(0.0, 1.0, (REACHABLE, lo.size)) * (hi - lo)
    a1 = lo + rng.uniform(0.0, 1.0, (REACHABLE, lo.size)) * (hi - lo)
    s = (PATH_POS[:frames] * step)[:, None, None]
    ang = (a0[None] + s * (a1 - a0)[None]).astype(np.float32).reshape(frames * REACHABLE, lo.size)
    ev = ikpso.BatchSolver(chain, 64, arith="reference", axis_mask=mask)
    pos = ev.evaluate(dev(ang))[1].cpu().numpy()
    ev.close()
    eff = [k - 1 for k in range(1, len(chain)) if chain["node_type"][k] == ikpso.NODE_EFFECTOR]
    near = pos[:, eff, :].reshape(frames, REACHABLE, len(eff), 3)
    d = rng.normal(size=(frames, B - REACHABLE, len(eff), 3))
    far = 10.0 * float(chain["length"][1:].sum()) * d / np.linalg.norm(d, axis=3, keepdims=True)
    return np.concatenate([near, far], axis=1).astype(np.float32)


def run_track(make, targets, stop, start=None, iterations=IT):
    """solve_track on a fresh solver: [angles, fitness, residual, iterations, states], kernel name."""
    s = make()
    nb = targets.shape[1]
    s.seed(nb)
    out = [t.cpu().numpy() for t in s.solve_track(dev(targets), start_pose=None if start is None else dev(start),
                                                  iterations=iterations, stop_fitness=stop)]
    out.append(s.generator_states(0, nb))
    name = s.kernel
    s.close()
    return out, name


def run_loop(make, targets, stop, start=None, iterations=IT):
    """The checker: one solve_until per frame on a fresh solver, each fed the previous answers."""
    s = make()
    nb = targets.shape[1]
    s.seed(nb)
    frames = [[], [], [], []]
    prev = None if start is None else dev(start)
    for t in range(targets.shape[0]):
        out = s.solve_until(dev(targets[t]), start_pose=prev, max_iterations=iterations,
                            stop_fitness=-1.0 if stop is None else stop)
        prev = out[0]
        for acc, o in zip(frames, out):
            acc.append(o.cpu().numpy())
    out = [np.stack(f) for f in frames]
    out.append(s.generator_states(0, nb))
    s.close()
    return out


def median_threshold(make, targets, rows=slice(0, REACHABLE), iterations=IT):
    return float(np.median(run_loop(make, targets, None, iterations=iterations)[1][:, rows]))


def assert_same(got, want):
    for name, g, w in zip(("angles", "fitness", "residual", "iterations", "generator states"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(bits(g), bits(w)), (name, np.argwhere(bits(g) != bits(w))[:8].tolist())


def check_track(make, targets, stop, start=None, iterations=IT):
    want = run_loop(make, targets, stop, start, iterations)
    got, name = run_track(make, targets, stop, start, iterations)
    nt, nb = targets.shape[:2]
    assert got[0].shape[:2] == (nt, nb) and got[3].shape == (nt, nb) and got[3].dtype == np.int32
    print("iterations:", got[3].tolist())
    assert_same(got, want)
    return got, want, name


@pytest.fixture(scope="module")
def scene_chain():
    return ikpso.reference_scene(reset=True).origin.to_cuda()


@pytest.fixture(scope="module")
def scene_targets(device, scene_chain):
    return path_targets(scene_chain)


# P = 65 on the resident kernel: two waves, the second nearly empty; P = 1024: a full workgroup;
# P = 300 on the streaming kernels (the host loop over the frames): two chunks
@pytest.mark.parametrize("kernel,P", [("resident", 65), ("resident", 1024), ("streaming", 300)])
@pytest.mark.parametrize("arith", ["reference", "fast"])
def test_families_and_sizes(device, scene_chain, scene_targets, arith, kernel, P):
    def make():
        return ikpso.BatchSolver(scene_chain, P, pso=PSO, arith=arith, kernel=kernel)

    got, _, name = check_track(make, scene_targets, median_threshold(make, scene_targets))
    assert kernel in name, name
    assert (got[3][:, REACHABLE:] == IT).all()


def test_routing(device, scene_chain, scene_targets):
    """A swarm of 2048 is routed to the cooperative family by AUTO: solve_track runs the streaming
    loop (and says so); a solver created for the cooperative kernels refuses."""
    P = 2048

    def make():
        return ikpso.BatchSolver(scene_chain, P, pso=PSO, kernel="auto")

    s = make()
    assert "coop" in s.kernel
    s.close()
    stop = median_threshold(lambda: ikpso.BatchSolver(scene_chain, P, pso=PSO, kernel="streaming"), scene_targets)
    want = run_loop(lambda: ikpso.BatchSolver(scene_chain, P, pso=PSO, kernel="streaming"), scene_targets, stop)
    got, name = run_track(make, scene_targets, stop)
    assert "streaming" in name, name
    assert_same(got, want)
    coop = ikpso.BatchSolver(scene_chain, P, pso=PSO, kernel="coop")
    coop.seed(B)
    with pytest.raises(ikpso.IkpsoError) as e:
        coop.solve_track(dev(scene_targets), iterations=IT, stop_fitness=stop)
    coop.close()
    assert e.value.status == ikpso._abi.IKPSO_ERR_UNSUPPORTED


def other_build(name):
    """(solver factory, chain, axis mask, expected kernel name part) of a resident FAST build at
    P = 128: the builds of tests/test_gpu_until.py::other_build, and the masked chain unfolded."""
    if name in ("dh", "nofold"):  # folded DH arm (axis mask) / the same chain on the Euler kernels
        wl = ikpso.workload("dh7" if name == "dh" else "dh7-nofold")
        return (lambda: ikpso.BatchSolver(wl.chain, 128, pso=PSO, fit=wl.fit, axis_mask=wl.axis_mask,
                                          fold=wl.fold, kernel="resident")), \
            wl.chain, wl.axis_mask, "dh7" if name == "dh" else "serial_tip11"
    if name == "colliders":
        wl = ikpso.workload(3)
        boxes = ikpso.init_colliders(4)[[0, 3]]
        return (lambda: ikpso.BatchSolver(wl.chain, 128, pso=PSO, colliders=boxes, kernel="resident")), \
            wl.chain, None, "ref_tree7"
    wl = ikpso.workload(5)  # 20-joint serial chain with soft limits: the 256-lane long-chain build
    return (lambda: ikpso.BatchSolver(wl.chain, 128, pso=PSO, fit=wl.fit, limit_weight=wl.limit_weight,
                                      soft_lo=wl.soft_lo, soft_hi=wl.soft_hi, kernel="resident")), \
        wl.chain, None, "serial_tip20"


@pytest.mark.parametrize("build", ["dh", "colliders", "serial20"])
def test_other_resident_builds(device, build):
    make, chain, mask, part = other_build(build)
    targets = path_targets(chain, mask)
    _, _, name = check_track(make, targets, median_threshold(make, targets))
    assert "resident" in name and part in name, name


def test_masked_chain_unfolded(device):
    """The Euler kernels skipping locked axes, start_pose=None: a locked dimension's rest value is
    the chain's in every frame, a free one's the previous answer."""
    make, chain, mask, part = other_build("nofold")
    assert any((int(m) & 7) not in (0, 7) for m in mask[1:])  # a node with a locked axis beside a free one
    targets = path_targets(chain, mask)
    got, _, name = check_track(make, targets, median_threshold(make, targets))
    assert "resident" in name and part in name, name
    assert got[0].shape[2] == 7


@pytest.mark.parametrize("arith", ["reference", "fast"])
def test_one_frame_is_solve_until(device, scene_chain, scene_targets, arith):
    def make():
        return ikpso.BatchSolver(scene_chain, 65, pso=PSO, arith=arith, kernel="resident")

    check_track(make, scene_targets[:1], median_threshold(make, scene_targets[:1]))


@pytest.mark.parametrize("arith", ["reference", "fast"])
def test_zero_iterations(device, scene_chain, scene_targets, arith):
    """No iteration in any frame: every frame's answer is its start pose, which in FAST (angles in
    revolutions) drifts through the radian round trip exactly as the loop's does."""
    def make():
        return ikpso.BatchSolver(scene_chain, 65, pso=PSO, arith=arith, kernel="resident")

    rng = np.random.default_rng(5)
    start = rng.uniform(0.1, 6.0, (B, 21)).astype(np.float32)
    got, _, _ = check_track(make, scene_targets, None, start=start, iterations=0)
    assert (got[3] == 0).all()
    if arith == "reference":
        assert np.array_equal(bits(got[0]), bits(np.broadcast_to(start, got[0].shape)))


@pytest.mark.parametrize("arith", ["reference", "fast"])
def test_negative_threshold_never_stops(device, scene_chain, scene_targets, arith):
    def make():
        return ikpso.BatchSolver(scene_chain, 65, pso=PSO, arith=arith, kernel="resident")

    got, _, _ = check_track(make, scene_targets, -1.0)
    assert (got[3] == IT).all()


@pytest.mark.parametrize("arith", ["reference", "fast"])
def test_early_stop(device, scene_chain, scene_targets, arith):
    """Conditions of the test, asserted on the checker's iteration counts: swarms stop mid-way at
    several counts, some frame needs no iteration, and no unreachable target ever stops."""
    def make():
        return ikpso.BatchSolver(scene_chain, 1024, pso=PSO, arith=arith, kernel="resident")

    stop = median_threshold(make, scene_targets)
    got, want, _ = check_track(make, scene_targets, stop)
    n = want[3]
    mid = n[:, :REACHABLE][(n[:, :REACHABLE] > 0) & (n[:, :REACHABLE] < IT)]
    assert mid.size >= 6 and len(set(mid.tolist())) >= 3, n.tolist()
    assert (n == 0).any(), n.tolist()
    assert (n[:, REACHABLE:] == IT).all(), n.tolist()
    # what the counts mean: a cell that stopped early met the threshold
    assert (got[1][n < IT] <= stop).all()


def test_evaluate_agrees_in_every_frame(device):
    """The collider build: evaluate() of a frame's answers, with that frame's start pose as the
    angle term's reference, is the fitness the frame reported."""
    make, chain, mask, _ = other_build("colliders")
    targets = path_targets(chain, mask)
    got, _ = run_track(make, targets, median_threshold(make, targets))
    ang, fit = got[0], got[1]
    s = make()
    for t in range(T):
        rest = None if t == 0 else dev(ang[t - 1])
        efit = s.evaluate(dev(ang[t]), dev(targets[t]), rest=rest)[0].cpu().numpy()
        assert np.array_equal(bits(efit), bits(fit[t])), t
    s.close()
