"""ikpso_solver_evaluate_gradient on the GPU (BatchSolver.gradient, BatchSolver.fitness): the fitness
ikpso_solver_evaluate_frames reports and its gradient with respect to the free angles.

Checker: tests/gradient64.py in float64 (the header's closed form assembled pair by pair, itself held to central
differences by tests/test_gradient64.py), ikpso_solver_evaluate_frames for the fitness, and the gradient
assembled on the host from ikpso_solver_evaluate_jacobian.  The tolerance on a gradient is, per term set (plain,
rotation, distance, penalty), four times the largest |gradient64 in float32 - gradient64 in float64| over that
set's cases: the spread of a valid fp32 evaluation with a margin of 4 for another operation order -- the
construction of tests/test_gpu_jacobian.py's `tols`.  No number is fixed in advance.
"""
import ctypes

import numpy as np
import pytest

import frames64
import gradient64
import ikpso
import topologies as tp
from gradient64 import Terms
from ikpso.dh import iiwa14

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 257                                # two workgroups of the kernel, the second holding one lane
NAMES = ("ref7", "serial6", "generic5", "generic1", "serial20", "iiwa14", "ref7coll")
ARITHS = ("fast", "reference")
MIXED = (1.0, 0.0, 0.5)                # cycled over the effectors (tests/test_gpu_evalframes.py)
FMAX = np.float32(np.finfo(np.float32).max)
OK, INVALID = ikpso._abi.IKPSO_OK, ikpso._abi.IKPSO_ERR_INVALID_ARG
SETS = {
    "plain": [(n, "plain") for n in NAMES],
    "rotation": [("ref7", "rotation"), ("generic5", "rotation"), ("iiwa14", "rotation")],
    "distance": [("ref7", "distance"), ("ref7", "distance_node_slot"), ("generic5", "distance"),
                 ("generic5", "distance_node_slot")],
    "penalty": [("ref7", "penalty"), ("generic5", "penalty")],
    # chains with a subtree that holds no weighted effector (section 3); held to the plain set's tolerance
    "bare": [("ref7bare", "plain"), ("generic5bare", "plain"), ("generic5bare", "penalty")],
}
KEYS = [k for keys in SETS.values() for k in keys]
SET_OF = {k: s for s, keys in SETS.items() for k in keys}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Case:
    """A chain, tests/test_gpu_evalframes.py's N in-bounds poses, rest poses and targets (the same seed, the
    same draws), one variant's terms; gradient64 and fitness64 in float64 and float32."""

    def __init__(self, name, variant, n=N, seed=41):
        self.name, self.variant, self.fit, self.mask, self.boxes = name, variant, ikpso.MAIN_FITNESS, None, None
        if name.startswith("ref7"):
            self.chain = ikpso.reference_scene(reset=True).origin.to_cuda()
            if name == "ref7coll":  # the collider fixture's two boxes (tests/test_tierb_fixtures.py)
                self.boxes = ikpso.init_colliders(4)[[0, 3]]
            if name == "ref7bare":  # two wrists of weight 0: nothing pulls on their joints
                self.chain["effector_weight"][[6, 7]] = 0.0
        elif name == "iiwa14":
            arm = iiwa14()
            self.chain, self.mask = arm.origin.to_cuda(), arm.axis_mask
        else:
            J = int(name.lstrip("abcdefghijklmnopqrstuvwxyz").rstrip("abcdefghijklmnopqrstuvwxyz"))
            self.chain = tp.serial(J) if name.startswith("serial") else tp.random_tree(J, 0)
            if name.endswith("bare"):  # the last leaf a plain node: a leaf that is no effector
                leaf = max(k for k in range(1, J + 1) if k not in self.chain["parent_index"].tolist())
                self.chain["node_type"][leaf] = ikpso.NODE
                self.chain["effector_weight"][leaf] = 0.0
        self.J, self.eff = len(self.chain) - 1, tp.effectors(self.chain)
        self.E, self.D = len(self.eff), len(tp.free_axes(self.chain, self.mask))
        rng = np.random.default_rng([seed, len(self.chain)])
        self.x, self.rest, other = (tp.random_poses(self.chain, n, rng, self.mask) for _ in range(3))
        p, R = frames64.effector_frames(self.chain, other, self.mask)
        self.targets, self.trot, self.rw = p.astype(np.float32), None, None
        self.terms = Terms(angle_weight=self.fit.angle_weight)
        extra = np.random.default_rng([seed, len(self.chain), 1])
        if variant.startswith("distance"):
            self.fit = ikpso.FitnessConfig(self.fit.angle_weight, 1.5, self.fit.error_threshold)
            reach = float(np.sum(np.abs(self.chain["length"][1:])))
            pos = np.concatenate([extra.uniform(-reach, reach, (self.J + 2, 3)), extra.uniform(0, 1, (self.J + 2, 1))], axis=1)
            self.terms.distance_weight, self.terms.positions = 1.5, pos.astype(np.float32).reshape(-1)
            self.terms.node_slot = variant == "distance_node_slot"
        if variant == "penalty":  # soft bounds a quarter of the clamp range inside the clamp bounds
            free = tp.free_axes(self.chain, self.mask)
            lo = np.array([self.chain["min_rotation"][k][c] for k, c in free], dtype=np.float64)
            hi = np.array([self.chain["max_rotation"][k][c] for k, c in free], dtype=np.float64)
            self.terms.limit_weight = 2.0
            self.terms.soft_lo, self.terms.soft_hi = (lo + 0.25 * (hi - lo)).astype(np.float32), (hi - 0.25 * (hi - lo)).astype(np.float32)
        if variant == "rotation":
            self.trot = R.astype(np.float32)
            self.rw = np.array([MIXED[e % 3] for e in range(self.E)], np.float32)
        args = (self.chain, self.x, self.rest, self.targets, self.terms, self.trot, self.rw, self.mask)
        self.g64 = gradient64.gradient64(*args)
        self.g32 = gradient64.gradient64(*args, dtype=np.float32).astype(np.float64)
        self.spread = float(np.max(np.abs(self.g32 - self.g64)))
        self.f64 = gradient64.fitness64(*args)
        self.f_spread = float(np.max(np.abs(gradient64.fitness64(*args, dtype=np.float32).astype(np.float64) - self.f64)))
        self.pulled = gradient64.subtree_has_effector(self.chain, self.mask)

    def solver(self, arith, P=64, **kw):
        if self.mask is not None:
            kw.setdefault("axis_mask", self.mask)
            kw.setdefault("kernel", "resident")  # FAST: the folded solver
        t = self.terms
        return ikpso.BatchSolver(self.chain, P, fit=self.fit, arith=arith, colliders=self.boxes, positions=t.positions,
                                 posref_node_slot=t.node_slot, limit_weight=t.limit_weight, soft_lo=t.soft_lo,
                                 soft_hi=t.soft_hi, **kw)

    def local32(self):
        """The angle and penalty part as the header rounds it, in float32: one product each, and their sum."""
        aw2 = np.float32(2.0) * (np.float32(self.fit.angle_weight) / np.float32(self.J))
        g = aw2 * (self.x - self.rest)
        if self.terms.penalised():
            lw2 = np.float32(2.0) * np.float32(self.terms.limit_weight)
            up, dn = self.x - self.terms.soft_hi, self.terms.soft_lo - self.x
            g = np.where(np.maximum(up, dn) > 0, g + np.where(up >= dn, lw2 * up, -(lw2 * dn)), g)
        assert g.dtype == np.float32
        return g


@pytest.fixture(scope="module")
def cases(device):
    return {key: Case(*key) for key in KEYS}


@pytest.fixture(scope="module")
def tols(cases):
    """One figure per term set: four times the largest |gradient64 in float32 - gradient64 in float64| over the
    set's cases; `fit` the same over every case's fitness (tests/test_gpu_evalframes.py's FLOOR)."""
    out = {}
    for name, keys in SETS.items():
        if name == "bare":
            continue
        per = {k: cases[k].spread for k in keys}
        out[name] = 4.0 * max(per.values())
        print(f"fp32 restatement of the {name} gradients against float64: " +
              ", ".join(f"{k[0]}/{k[1]} {v:.3e}" for k, v in per.items()) + f"; tolerance {out[name]:.3e}")
    out["bare"] = out["plain"]
    out["fit"] = 4.0 * max(c.f_spread for c in cases.values())
    print(f"fp32 restatement of the fitness against float64, max over every case: tolerance {out['fit']:.3e}")
    return out


@pytest.fixture(scope="module")
def runs(cases):
    """Every (case, arithmetic) once: the batch, its first vector alone, evaluate_frames' fitness, positions and
    rotations and evaluate's fitness for the same arguments, and the Jacobians."""
    out = {}
    for key, case in cases.items():
        for arith in ARITHS:
            s = case.solver(arith)
            x, tg, rest = dev(case.x), dev(case.targets), dev(case.rest)
            trot = None if case.trot is None else dev(case.trot)
            fit, grad = s.gradient(x, tg, rest, trot, case.rw)
            fit1, grad1 = s.gradient(x[:1], tg[:1], rest[:1], None if trot is None else trot[:1], case.rw)
            ffit, fpos, frot, _ = s.evaluate_frames(x, tg, rest, trot, case.rw)
            efit, _ = s.evaluate(x, tg, rest)
            jac, _ = s.jacobian(x)
            r = dict(fit=fit, grad=grad, fit1=fit1, grad1=grad1, ffit=ffit, fpos=fpos, frot=frot, efit=efit, jac=jac)
            if case.trot is not None:
                r["zero"] = s.gradient(x, tg, rest, trot, np.zeros(case.E, np.float32))[1]
                r["null"] = s.gradient(x, tg, rest)[1]
                if (case.rw == 0).any():  # an effector of weight 0 never has its target read
                    poison = case.trot.copy()
                    poison[:, case.rw == 0] = np.nan
                    r["nan_fit"], r["nan_grad"] = s.gradient(x, tg, rest, dev(poison), case.rw)
            out[key + (arith,)] = {k: v.cpu().numpy() for k, v in r.items()}
            s.close()
    return out


def params(keys=KEYS):
    return [k + (a,) for k in keys for a in ARITHS]


# ---------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("name,variant,arith", params())
def test_values(cases, runs, tols, name, variant, arith):
    """Measured on an MI355X, worst |g_gpu - gradient64| per term set (tolerance: four times the set's largest
    spread, each time the reference tree's, whose gradients reach 67): plain 1.19e-5 REFERENCE, 2.45e-5 FAST
    (tolerance 3.678e-5); rotation 1.03e-5, 2.53e-5 (4.266e-5); distance 1.43e-5, 3.19e-5 (4.620e-5, the node
    slot); penalty 1.19e-5, 2.45e-5 (3.678e-5).  Serial 20: 2.4e-6 REFERENCE, 5.8e-6 FAST.  No FAST build needed
    an allowance for the hardware sin/cos."""
    case, r = cases[(name, variant)], runs[(name, variant, arith)]
    tol = tols[SET_OF[(name, variant)]]
    g = r["grad"]
    assert g.shape == (N, case.D) and g.dtype == np.float32
    if name == "iiwa14":
        assert case.D == 7  # a masked chain returns its free dimensions
    e = float(np.max(np.abs(g.astype(np.float64) - case.g64)))
    print(f"{name}/{variant} {arith}: D={case.D} |gradient64| up to {np.max(np.abs(case.g64)):.3e}, max |g_gpu - gradient64| = "
          f"{e:.3e} (tolerance {tol:.3e}; four times this case's own spread {4 * case.spread:.3e})")
    assert np.isfinite(g).all()
    assert e <= tol


@pytest.mark.parametrize("name,variant,arith", params())
def test_fitness_is_evaluate_frames(cases, runs, tols, name, variant, arith):
    case, r = cases[(name, variant)], runs[(name, variant, arith)]
    hit = r["efit"] == FMAX
    assert not hit.any() or case.boxes is not None
    assert np.array_equal(r["fit"] == FMAX, hit)
    d = np.abs(r["fit"].astype(np.float64) - r["ffit"].astype(np.float64))[~hit]
    d64 = np.abs(r["fit"].astype(np.float64) - case.f64)[~hit]
    print(f"{name}/{variant} {arith}: max |fitness - evaluate_frames'| = {d.max():.3e}, max |fitness - fitness64| = "
          f"{d64.max():.3e}, floor {tols['fit']:.3e}")
    if arith == "reference":
        assert np.array_equal(bits(r["fit"]), bits(r["ffit"]))
    else:
        assert (d <= tols["fit"]).all()


# ------------------------------------------------------------------------------ 2. the Jacobian route
@pytest.mark.parametrize("name,variant,arith", params([k for k in KEYS if not k[1].startswith("distance")]))
def test_jacobian_route(cases, runs, tols, name, variant, arith):
    """The gradient assembled in float64 on the host from ikpso_solver_evaluate_jacobian's Jacobians and
    ikpso_solver_evaluate_frames' positions and rotations (no distance term: it has no columns for it)."""
    case, r = cases[(name, variant)], runs[(name, variant, arith)]
    jac = r["jac"].astype(np.float64)
    w = case.chain["effector_weight"][case.eff].astype(np.float64)
    p = r["fpos"].astype(np.float64)[:, case.eff - 1]
    g = np.einsum("nei,neid->nd", 2.0 * w[None, :, None] * (p - case.targets.astype(np.float64)), jac[:, :, 0:3])
    if case.trot is not None:
        M = r["frot"].astype(np.float64)[:, case.eff - 1] @ np.swapaxes(case.trot.astype(np.float64), -1, -2)
        v = np.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], axis=-1)
        g += np.einsum("nei,neid->nd", 2.0 * (w * case.rw.astype(np.float64))[None, :, None] * v, jac[:, :, 3:6])
    local = gradient64.gradient64(case.chain, case.x, case.rest, case.targets, case.terms, mask=case.mask, parts=True)
    g += local["angle"] + local["penalty"]
    tol = tols[SET_OF[(name, variant)]]
    e = float(np.max(np.abs(r["grad"].astype(np.float64) - g)))
    print(f"{name}/{variant} {arith}: max |g_gpu - gradient by the Jacobian route| = {e:.3e} (tolerance {tol:.3e})")
    assert e <= tol


# ------------------------------------------------------------------------------------- 3. structure
@pytest.mark.parametrize("name,variant,arith", params(SETS["bare"]))
def test_a_dimension_nothing_pulls_on(cases, runs, name, variant, arith):
    """A free dimension whose subtree holds no weighted effector gets exactly the angle and penalty part."""
    case, g = cases[(name, variant)], runs[(name, variant, arith)]["grad"]
    bare = ~case.pulled
    assert bare.any() and case.pulled.any()
    want = case.local32()
    assert (g[:, bare] == want[:, bare]).all()  # ==: signed zero ignored
    assert not (g[:, case.pulled] == want[:, case.pulled]).all()
    if variant == "penalty":
        beyond = (case.x > case.terms.soft_hi) | (case.x < case.terms.soft_lo)
        assert beyond[:, bare].any() and (~beyond[:, bare]).any()


@pytest.mark.parametrize("name,variant,arith", params(SETS["rotation"]))
def test_rotation_weights_of_zero(cases, runs, name, variant, arith):
    """Every weight 0 with a target_rot, and NULL weights: the plain case's bits.  A NaN-filled target of a
    weight-0 effector is never read."""
    case, r = cases[(name, variant)], runs[(name, variant, arith)]
    plain = runs[(name, "plain", arith)]["grad"]
    assert np.array_equal(bits(r["zero"]), bits(plain)) and np.array_equal(bits(r["null"]), bits(plain))
    assert not np.array_equal(bits(r["grad"]), bits(plain))
    if name == "ref7":
        assert (case.rw == 0).any()
    if (case.rw == 0).any():
        assert np.isfinite(r["nan_grad"]).all() and np.isfinite(r["nan_fit"]).all()
        assert np.array_equal(bits(r["nan_grad"]), bits(r["grad"])) and np.array_equal(bits(r["nan_fit"]), bits(r["fit"]))


# ----------------------------------------------------------------------------------- 4. launch shape
@pytest.mark.parametrize("name,variant,arith", params())
def test_one_vector_alone(runs, name, variant, arith):
    r = runs[(name, variant, arith)]
    assert np.array_equal(bits(r["grad1"]), bits(r["grad"][:1]))
    assert np.array_equal(bits(r["fit1"]), bits(r["fit"][:1]))


def test_grid_stride(cases, runs):
    """2^21 + 1 vectors, the case's N poses over and over: past the grid cap's 8192 x 256 lanes, so the last one
    is a second trip of lane 0.  Every vector has the batch's bits."""
    case, r = cases[("ref7", "rotation")], runs[("ref7", "rotation", "fast")]
    n = 8192 * 256 + 1
    idx = torch.arange(n, device="cuda") % N
    x, tg, rest, trot = (dev(a)[idx].contiguous() for a in (case.x, case.targets, case.rest, case.trot))
    s = case.solver("fast")
    fit, grad = s.gradient(x, tg, rest, trot, case.rw)
    torch.cuda.synchronize()
    s.close()
    assert torch.equal(grad.view(torch.int32), dev(r["grad"]).view(torch.int32)[idx])
    assert torch.equal(fit.view(torch.int32), dev(r["fit"]).view(torch.int32)[idx])


def test_other_solver_families(cases, runs):
    """A cooperative and a streaming solver return the resident solver's bits."""
    case, r = cases[("ref7", "rotation")], runs[("ref7", "rotation", "fast")]
    x, tg, rest, trot = dev(case.x), dev(case.targets), dev(case.rest), dev(case.trot)
    for kw in (dict(kernel="coop", P=2048), dict(kernel="streaming")):
        s = case.solver("fast", **kw)
        fit, grad = s.gradient(x, tg, rest, trot, case.rw)
        s.close()
        assert np.array_equal(bits(grad.cpu().numpy()), bits(r["grad"])), kw
        assert np.array_equal(bits(fit.cpu().numpy()), bits(r["fit"])), kw


# ------------------------------------------------------------------------------------- 5. colliders
@pytest.mark.parametrize("arith", ARITHS)
def test_colliders(cases, runs, tols, oracle, arith):
    """FLT_MAX exactly where evaluate says so; the gradient is the collider-free solver's, finite everywhere."""
    case, r, free = cases[("ref7coll", "plain")], runs[("ref7coll", "plain", arith)], runs[("ref7", "plain", arith)]
    assert np.array_equal(case.x, cases[("ref7", "plain")].x)
    ohit = np.array([oracle.fitness(case.chain, v, colliders=case.boxes) for v in case.x], dtype=np.float32) == FMAX
    assert 0 < ohit.sum() < N  # the reference alone: at least one colliding and one free pose
    hit = r["efit"] == FMAX
    print(f"ref7coll {arith}: {int(hit.sum())} of {N} poses touch a box (oracle: {int(ohit.sum())})")
    assert 0 < hit.sum() < N
    if arith == "reference":
        assert np.array_equal(hit, ohit)
    assert np.array_equal(r["fit"] == FMAX, hit) and np.isfinite(r["fit"][~hit]).all()
    assert np.isfinite(r["grad"]).all()
    e = np.abs(r["grad"].astype(np.float64) - free["grad"].astype(np.float64))
    print(f"ref7coll against ref7, {arith}: max gradient difference {e.max():.3e} (colliding poses {e[hit].max():.3e}), "
          f"tolerance {tols['plain']:.3e}")
    assert e.max() <= tols["plain"]


# -------------------------------------------------------------------------------------- 6. statuses
def test_statuses_and_the_empty_call(cases):
    case = cases[("ref7", "rotation")]
    s = case.solver("fast")
    n, E = 4, case.E
    x, trot = dev(case.x[:n]), dev(case.trot[:n])
    sentinel = -12345.0
    fit = torch.full((n,), sentinel, dtype=torch.float32, device="cuda")
    grad = torch.full((n, case.D), sentinel, dtype=torch.float32, device="cuda")
    fn = s._lib.ikpso_solver_evaluate_gradient

    def call(weights, rot=True, count=n, angles=True, out=True, handle=True):
        w = None if weights is None else (ctypes.c_float * E)(*weights)
        st = fn(s._h if handle else None, x.data_ptr() if angles else None, None, None, trot.data_ptr() if rot else None,
                w, count, fit.data_ptr(), grad.data_ptr() if out else None, None)
        torch.cuda.synchronize()
        return st

    for bad in (-1.0, float("nan"), float("inf")):
        assert call((1.0, bad, 0.0)) == INVALID, bad
        assert call((0.0, 0.0, bad), rot=False) == INVALID, bad
    assert call((0.0, 0.5, 0.0), rot=False) == INVALID   # a weight > 0 needs target_rot
    assert call((1.0, 1.0, 1.0), count=-1) == INVALID
    assert call((1.0, 1.0, 1.0), angles=False) == INVALID
    assert call((1.0, 1.0, 1.0), out=False) == INVALID   # out_gradient is required
    assert call(None, rot=False, out=False) == INVALID
    assert call((1.0, 1.0, 1.0), handle=False) == INVALID
    assert call((1.0, 1.0, 1.0), count=0) == OK          # no device work ...
    assert fn(s._h, None, None, None, None, None, 0, None, None, None) == OK
    assert bool((fit == sentinel).all()) and bool((grad == sentinel).all())  # ... and nothing refused wrote anything
    assert call((0.0, 0.0, 0.0), rot=False) == OK        # all weights 0 reads no target_rot
    assert bool((fit != sentinel).all()) and bool((grad != sentinel).all())
    fit.fill_(sentinel)
    assert fn(s._h, x.data_ptr(), None, None, None, None, n, None, grad.data_ptr(), None) == OK  # out_fitness is optional
    torch.cuda.synchronize()
    assert bool((fit == sentinel).all())
    s.close()


def test_a_pending_cooperative_solve_is_left_alone(cases, runs, monkeypatch):
    """The call neither settles nor disturbs a pending cooperative solve: with every group wait giving up
    (IKPSO_COOP_SPIN_LIMIT=0, tests/test_gpu_coop.py) the unsettled answers read NaN before and after the call,
    no fallback is counted until sync(), and sync() then gives what it gives without the call."""
    case, want = cases[("ref7", "plain")], runs[("ref7", "plain", "reference")]
    B, P, I = 1, 16384, 5
    tg = dev(case.targets[:B])
    x, targets, rest = dev(case.x), dev(case.targets), dev(case.rest)
    monkeypatch.setenv("IKPSO_COOP_SPIN_LIMIT", "0")
    answers = []
    for between in (True, False):
        s = case.solver("reference", P, pso=ikpso.PSOConfig(0.5, 0.5, 1.25, I), kernel="coop")
        s.seed(B)
        a0, f0, _ = s.solve(tg, iterations=I, sync=False)
        torch.cuda.synchronize()
        assert torch.isnan(f0).any()
        before = s.fallbacks
        if between:
            fit, grad = s.gradient(x, targets, rest)
            torch.cuda.synchronize()
            assert np.array_equal(bits(grad.cpu().numpy()), bits(want["grad"]))
            assert np.array_equal(bits(fit.cpu().numpy()), bits(want["fit"]))
            assert s.fallbacks == before and torch.isnan(f0).any()  # still pending
        s.sync()
        assert s.fallbacks == before + 1
        answers.append((a0.cpu().numpy(), f0.cpu().numpy()))
        s.close()
    assert np.isfinite(answers[0][1]).all()
    assert np.array_equal(bits(answers[0][0]), bits(answers[1][0])) and np.array_equal(bits(answers[0][1]), bits(answers[1][1]))


# -------------------------------------------------------------------------------------- 7. autograd
def test_autograd(cases, runs):
    case, r = cases[("ref7", "rotation")], runs[("ref7", "rotation", "fast")]
    s = case.solver("fast")
    tg, rest, trot = dev(case.targets), dev(case.rest), dev(case.trot)
    x = dev(case.x).requires_grad_(True)
    f = s.fitness(x, tg, rest, trot, case.rw)
    assert f.requires_grad and f.shape == (N,)
    assert np.array_equal(bits(f.detach().cpu().numpy()), bits(r["fit"]))
    f.sum().backward()
    assert np.array_equal(bits(x.grad.cpu().numpy()), bits(r["grad"]))
    x.grad = None
    scale = torch.linspace(-2.0, 3.0, N, device="cuda")
    (s.fitness(x, tg, rest, trot, case.rw) * scale).sum().backward()
    assert torch.equal(x.grad, scale[:, None] * dev(r["grad"]))
    assert tg.grad is None and rest.grad is None
    s.close()
