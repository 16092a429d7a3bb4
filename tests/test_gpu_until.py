"""BatchSolver.solve_until (ikpso_solve_batch_until) on the GPU: per-swarm early stop at a
fitness threshold, in the resident and the streaming kernels.

The statement under test is exact: a swarm that stops after n iterations leaves the
outputs and generator states of solve(iterations=n), bit for bit, and n is the first
iteration count at which the global best meets the threshold.  The stopping kernels are
the plain kernels' source with the stop compiled in (resident) or switched on by a
run-time field (streaming), so this is asserted in FAST arithmetic as in REFERENCE; every
comparison below is on bit patterns.

The threshold never comes from the code under test: it is the median fitness the
reachable swarms have after a plain solve(iterations=30).
"""
import numpy as np
import pytest

import ikpso

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, REACHABLE, MAX_IT = 24, 16, 60
PSO = ikpso.PSOConfig(0.5, 0.5, 1.25, MAX_IT)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module")
def scene_chain():
    return ikpso.reference_scene(reset=True).origin.to_cuda()


@pytest.fixture(scope="module")
def scene_targets(device, scene_chain):
    """[24, 3, 3]: 16 reachable targets (the effector positions evaluate() returns for random
    in-bounds angle vectors), then 8 at ten times the arm's reach."""
    rng = np.random.default_rng(2024)
    lo, hi = scene_chain["min_rotation"][1:].reshape(-1), scene_chain["max_rotation"][1:].reshape(-1)
    ang = (lo + rng.uniform(0.0, 1.0, (REACHABLE, lo.size)) * (hi - lo)).astype(np.float32)
    s = ikpso.BatchSolver(scene_chain, 64, arith="reference")
    pos = s.evaluate(dev(ang))[1].cpu().numpy()
    s.close()
    eff = [k - 1 for k in range(1, len(scene_chain)) if scene_chain["node_type"][k] == ikpso.NODE_EFFECTOR]
    assert len(eff) == 3
    reach = float(scene_chain["length"][1:5].sum() + scene_chain["length"][5:].max())  # origin to an effector
    d = rng.normal(size=(B - REACHABLE, 3, 3))
    far = 10.0 * reach * d / np.linalg.norm(d, axis=2, keepdims=True)
    return np.concatenate([pos[:, eff, :], far]).astype(np.float32)


class Runner:
    """One solver configuration: solve_until once, plain solves of any length (a second
    solver, re-seeded for every run, so each starts from fresh generator states)."""

    def __init__(self, make, targets, nb=B):
        self.make, self.tg, self.nb = make, dev(targets), nb
        self.plain_solver = make()
        self.cache = {}

    def plain(self, n, start=None):
        if start is None and n in self.cache:
            return self.cache[n]
        s = self.plain_solver
        s.seed(self.nb)
        out = [t.cpu().numpy() for t in s.solve(self.tg, start_pose=start, iterations=n)]
        out.append(s.generator_states(0, self.nb).reshape(self.nb, s.P, -1))
        if start is None:
            self.cache[n] = out
        return out

    def until(self, stop, start=None, max_it=MAX_IT):
        s = self.make()
        s.seed(self.nb)
        out = [t.cpu().numpy() for t in s.solve_until(self.tg, start_pose=start, max_iterations=max_it,
                                                      stop_fitness=stop)]
        out.append(s.generator_states(0, self.nb).reshape(self.nb, s.P, -1))
        self.kernel = s.kernel
        s.close()
        return out

    def threshold(self, rows=slice(0, REACHABLE)):
        return float(np.median(self.plain(30)[1][rows]))

    def close(self):
        self.plain_solver.close()


def check_truncation(r, stop, max_it=MAX_IT):
    """solve_until against plain solves of every iteration count it reports.  Returns the counts."""
    ang, fit, res, its, states = r.until(stop, max_it=max_it)
    assert its.dtype == np.int32 and its.min() >= 0 and its.max() <= max_it
    for n in sorted(set(its.tolist())):
        rows = its == n
        pang, pfit, pres, pstates = r.plain(n)
        assert np.array_equal(bits(ang[rows]), bits(pang[rows])), n
        assert np.array_equal(bits(fit[rows]), bits(pfit[rows])), n
        assert np.array_equal(bits(res[rows]), bits(pres[rows])), n
        assert np.array_equal(states[rows], pstates[rows]), n
        if n < max_it:
            assert (fit[rows] <= stop).all(), n
        else:  # ran to the maximum
            assert (fit[rows] > stop).all(), n
        if n > 0:  # minimality: one iteration earlier the threshold was not met
            assert (r.plain(n - 1)[1][rows] > stop).all(), n
    return its


def check_scene_conditions(its):
    """Conditions of the test (not measurements): enough swarms stop mid-way, at several
    iteration counts, and no unreachable target stops."""
    mid = its[(its > 0) & (its < MAX_IT)]
    print("iterations:", its.tolist())
    assert mid.size >= 4 and len(set(mid.tolist())) >= 3, its
    assert (its[REACHABLE:] == MAX_IT).all(), its


# P = 65 on the resident kernel: two waves, the second nearly empty; P = 300 on the streaming
# kernels: two chunks, the second partly filled; P = 1024: full workgroup / four chunks.
CASES = [("resident", 65), ("streaming", 300), ("resident", 1024), ("streaming", 1024)]


@pytest.mark.parametrize("kernel,P", CASES)
@pytest.mark.parametrize("arith", ["reference", "fast"])
def test_truncation_parity(device, scene_chain, scene_targets, arith, kernel, P):
    r = Runner(lambda: ikpso.BatchSolver(scene_chain, P, pso=PSO, arith=arith, kernel=kernel), scene_targets)
    its = check_truncation(r, r.threshold())
    assert kernel in r.kernel, r.kernel
    r.close()
    check_scene_conditions(its)


@pytest.mark.parametrize("kernel,P", [("resident", 65), ("streaming", 300)])
@pytest.mark.parametrize("arith", ["reference", "fast"])
def test_disabled_stop(device, scene_chain, scene_targets, arith, kernel, P):
    """A negative threshold never stops: solve(iterations=60) bit for bit, every count 60."""
    r = Runner(lambda: ikpso.BatchSolver(scene_chain, P, pso=PSO, arith=arith, kernel=kernel), scene_targets)
    ang, fit, res, its, states = r.until(-1.0)
    pang, pfit, pres, pstates = r.plain(MAX_IT)
    r.close()
    assert (its == MAX_IT).all()
    assert np.array_equal(bits(ang), bits(pang)) and np.array_equal(bits(fit), bits(pfit))
    assert np.array_equal(bits(res), bits(pres)) and np.array_equal(states, pstates)


@pytest.mark.parametrize("kernel,P", [("resident", 65), ("streaming", 300)])
@pytest.mark.parametrize("arith", ["reference", "fast"])
def test_zero_iterations(device, scene_chain, scene_targets, arith, kernel, P):
    """Warm start at the answers of an earlier solve with a threshold above their evaluated
    fitness: no swarm runs an iteration, the particles have drawn their D initial values only."""
    r = Runner(lambda: ikpso.BatchSolver(scene_chain, P, pso=PSO, arith=arith, kernel=kernel), scene_targets)
    start = dev(r.plain(30)[0])
    efit = r.plain_solver.evaluate(start, r.tg, rest=start)[0].cpu().numpy()
    stop = 1.05 * float(efit.max()) + 1e-3
    ang, fit, res, its, states = r.until(stop, start=start)
    pang, pfit, pres, pstates = r.plain(0, start=start)
    r.close()
    assert (its == 0).all()
    assert np.array_equal(states, pstates)
    assert np.array_equal(bits(ang), bits(pang)) and np.array_equal(bits(fit), bits(pfit))
    if arith == "reference":
        assert np.array_equal(bits(ang), bits(start.cpu().numpy()))


def test_families_agree(device, scene_chain, scene_targets):
    """REFERENCE, P = 1024: the resident and the streaming kernels stop every swarm at the same
    iteration with the same answer."""
    out = {}
    for kernel in ("resident", "streaming"):
        r = Runner(lambda: ikpso.BatchSolver(scene_chain, 1024, pso=PSO, arith="reference", kernel=kernel),
                   scene_targets)
        stop = r.threshold()
        out[kernel] = (stop, r.until(stop))
        r.close()
    (sa, a), (sb, b) = out["resident"], out["streaming"]
    assert sa == sb
    assert np.array_equal(a[3], b[3])
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert ((a[3] > 0) & (a[3] < MAX_IT)).sum() >= 4


def test_routing(device, scene_chain, scene_targets):
    """A swarm of 2048 is routed to the cooperative family by AUTO: solve_until runs it on the
    streaming kernels (and says so); a solver created for the cooperative kernels refuses."""
    P = 2048
    auto = ikpso.BatchSolver(scene_chain, P, pso=PSO, kernel="auto")
    assert "coop" in auto.kernel
    r = Runner(lambda: ikpso.BatchSolver(scene_chain, P, pso=PSO, kernel="streaming"), scene_targets)
    stop = r.threshold()
    want = r.until(stop)
    r.close()
    auto.seed(B)
    got = [t.cpu().numpy() for t in auto.solve_until(dev(scene_targets), max_iterations=MAX_IT, stop_fitness=stop)]
    assert "streaming" in auto.kernel, auto.kernel
    got.append(auto.generator_states(0, B).reshape(B, P, -1))
    auto.close()
    assert np.array_equal(got[3], want[3]) and ((got[3] > 0) & (got[3] < MAX_IT)).any()
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w))
    coop = ikpso.BatchSolver(scene_chain, P, pso=PSO, kernel="coop")
    coop.seed(B)
    with pytest.raises(ikpso.IkpsoError) as e:
        coop.solve_until(dev(scene_targets), max_iterations=MAX_IT, stop_fitness=stop)
    coop.close()
    assert e.value.status == ikpso._abi.IKPSO_ERR_UNSUPPORTED


def other_build(name):
    """(solver factory, targets, expected kernel name part) of a resident FAST build at P = 128."""
    if name == "dh":  # folded DH arm: axis mask, 8 waves per SIMD, two swarms per CU
        wl = ikpso.workload("dh7")
        return (lambda: ikpso.BatchSolver(wl.chain, 128, pso=PSO, fit=wl.fit, axis_mask=wl.axis_mask,
                                          kernel="resident")), wl.targets(0, B), "dh7"
    if name == "colliders":  # the collider build's iteration re-reads the chain constants (kernarg_cc)
        wl = ikpso.workload(3)
        boxes = ikpso.init_colliders(4)[[0, 3]]
        return (lambda: ikpso.BatchSolver(wl.chain, 128, pso=PSO, colliders=boxes, kernel="resident")), \
            wl.targets(0, B), "ref_tree7"
    wl = ikpso.workload(5)  # 20-joint serial chain: the 256-lane long-chain build
    return (lambda: ikpso.BatchSolver(wl.chain, 128, pso=PSO, fit=wl.fit, limit_weight=wl.limit_weight,
                                      soft_lo=wl.soft_lo, soft_hi=wl.soft_hi, kernel="resident")), \
        wl.targets(0, B), "serial_tip20"


@pytest.mark.parametrize("build", ["dh", "colliders", "serial20"])
def test_other_resident_builds(device, build):
    """Truncation parity of the other resident builds, FAST, P = 128.  The threshold is the
    median fitness of all swarms after 30 iterations, so about half stop by then."""
    make, targets, name = other_build(build)
    r = Runner(make, targets)
    stop = r.threshold(slice(None))
    its = check_truncation(r, stop)
    assert "resident" in r.kernel and name in r.kernel, r.kernel
    r.close()
    print("iterations:", its.tolist())
    assert ((its > 0) & (its < MAX_IT)).sum() >= 4, its


def test_evaluate_agrees_on_stopped_rows(device):
    """evaluate() of a stopped swarm's answer is its reported fitness, as for plain solves of the
    collider builds (test_gpu_collide.py: one arithmetic in the solve and in the evaluate kernel)."""
    make, targets, _ = other_build("colliders")
    r = Runner(make, targets)
    stop = r.threshold(slice(None))
    ang, fit, res, its, _ = r.until(stop)
    efit = r.plain_solver.evaluate(dev(ang), r.tg)[0].cpu().numpy()
    r.close()
    stopped = its < MAX_IT
    assert stopped.sum() >= 4
    assert np.array_equal(bits(efit[stopped]), bits(fit[stopped]))
