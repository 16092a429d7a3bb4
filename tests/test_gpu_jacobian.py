"""ikpso_solver_evaluate_jacobian on the GPU (BatchSolver.jacobian): the geometric Jacobian of every effector
and the node positions, for given angle vectors.

Checker: tests/jacobian64.py in float64 (the header's definition in numpy, itself held to central differences
by tests/test_jacobian64.py), and ikpso_solver_evaluate for the positions.  Every tolerance on a value is four
times what a float32 restatement of the same numpy expression differs from float64 by, over every case's own
poses: the spread of a valid fp32 evaluation with a margin of 4 for another operation order -- the
construction of tests/test_gpu_evalframes.py's `floors`.  No number is fixed in advance.
"""
import numpy as np
import pytest

import frames64
import ikpso
import jacobian64
import topologies as tp
from ikpso.dh import iiwa14

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 257                                # two workgroups of the kernel, the second holding one lane
NAMES = ("ref7", "serial6", "generic5", "generic1", "serial20", "iiwa14", "ref7coll")
ARITHS = ("fast", "reference")
OK, INVALID = ikpso._abi.IKPSO_OK, ikpso._abi.IKPSO_ERR_INVALID_ARG


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Case:
    """A chain and N in-bounds poses (tests/test_gpu_evalframes.py's, by the same seed); the float64 Jacobian
    and positions and the float32 restatement's spread."""

    def __init__(self, name, n=N, seed=41):
        self.name, self.mask, self.boxes = name, None, None
        if name.startswith("ref7"):
            self.chain = ikpso.reference_scene(reset=True).origin.to_cuda()
            if name == "ref7coll":  # the collider fixture's two boxes (tests/test_tierb_fixtures.py)
                self.boxes = ikpso.init_colliders(4)[[0, 3]]
        elif name == "iiwa14":
            arm = iiwa14()
            self.chain, self.mask = arm.origin.to_cuda(), arm.axis_mask
        else:
            J = int(name.lstrip("abcdefghijklmnopqrstuvwxyz"))
            self.chain = tp.serial(J) if name.startswith("serial") else tp.random_tree(J, 0)
        self.J, self.eff = len(self.chain) - 1, tp.effectors(self.chain)
        self.E, self.free = len(self.eff), tp.free_axes(self.chain, self.mask)
        self.D = len(self.free)
        rng = np.random.default_rng([seed, len(self.chain)])
        self.x = tp.random_poses(self.chain, n, rng, self.mask)
        self.J64 = jacobian64.effector_jacobian(self.chain, self.x, self.mask)
        J32 = jacobian64.effector_jacobian(self.chain, self.x, self.mask, dtype=np.float32).astype(np.float64)
        self.lin_spread = float(np.max(np.abs(J32 - self.J64)[:, :, 0:3]))
        self.ang_spread = float(np.max(np.abs(J32 - self.J64)[:, :, 3:6]))
        full = tp.expand(self.chain, self.x, self.mask)
        self.p64, _ = frames64.node_frames(self.chain, full)
        p32, _ = frames64.node_frames(self.chain, full, dtype=np.float32)
        self.pos_spread = float(np.max(np.abs(p32.astype(np.float64) - self.p64)))
        # [E, D]: is free dimension d an angle of effector e's node or of one of its ancestors?
        self.on_path = np.array([[k in jacobian64.ancestors(self.chain, int(m)) for k, _ in self.free]
                                 for m in self.eff])

    def solver(self, arith, P=64, **kw):
        if self.mask is not None:
            kw.setdefault("axis_mask", self.mask)
            kw.setdefault("kernel", "resident")  # FAST: the folded solver
        return ikpso.BatchSolver(self.chain, P, arith=arith, colliders=self.boxes, **kw)


@pytest.fixture(scope="module")
def cases(device):
    return {name: Case(name) for name in NAMES}


@pytest.fixture(scope="module")
def tols(cases):
    """One figure each for the linear rows, the angular rows and the positions: four times the largest
    |float32 numpy evaluation - float64| over every case's poses.  The cases' own spreads are printed."""
    out = {}
    for what in ("lin", "ang", "pos"):
        per = {n: getattr(c, what + "_spread") for n, c in cases.items()}
        out[what] = 4.0 * max(per.values())
        print(f"fp32 restatement of {what} against float64: " + ", ".join(f"{n} {v:.3e}" for n, v in per.items()) +
              f"; tolerance {out[what]:.3e}")
    return out


@pytest.fixture(scope="module")
def runs(cases):
    """Every (case, arithmetic) once: the batch, its first vector alone, and evaluate()'s positions."""
    out = {}
    for name, case in cases.items():
        for arith in ARITHS:
            s = case.solver(arith)
            x = dev(case.x)
            jac, pos = s.jacobian(x)
            jac1, pos1 = s.jacobian(x[:1])
            _, epos = s.evaluate(x)
            out[(name, arith)] = dict(jac=jac.cpu().numpy(), pos=pos.cpu().numpy(), jac1=jac1.cpu().numpy(),
                                      pos1=pos1.cpu().numpy(), epos=epos.cpu().numpy())
            s.close()
    return out


def params():
    return [(n, a) for n in NAMES for a in ARITHS]


# ---------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("name,arith", params())
def test_values(cases, runs, tols, name, arith):
    """Measured on an MI355X.  Linear rows (tolerance 3.525e-6, four times serial6's spread of 8.813e-7, the
    largest): worst |J_gpu - J_float64| 9.60e-7 REFERENCE (ref7), 2.60e-6 FAST (ref7coll; ref7 2.58e-6, serial20
    1.52e-6).  Angular rows (tolerance 1.986e-6, four times serial20's spread of 4.965e-7): worst 5.36e-7
    REFERENCE, 1.36e-6 FAST (both serial20), the FAST axes taken from the compensated rotation.  Axis norms
    are within 7.9e-7 of 1 (serial20 FAST)."""
    case, jac = cases[name], runs[(name, arith)]["jac"].astype(np.float64)
    e = np.abs(jac - case.J64)
    lin, ang = float(e[:, :, 0:3].max()), float(e[:, :, 3:6].max())
    print(f"{name} {arith}: D={case.D} E={case.E} max |J_gpu - J_float64| linear {lin:.3e} (tolerance {tols['lin']:.3e}, "
          f"four times this case's own spread: {4 * case.lin_spread:.3e}), angular {ang:.3e} (tolerance "
          f"{tols['ang']:.3e}, own: {4 * case.ang_spread:.3e})")
    assert np.isfinite(jac).all()
    assert lin <= tols["lin"]
    assert ang <= tols["ang"]


# ------------------------------------------------------------------------------------- 2. structure
@pytest.mark.parametrize("name,arith", params())
def test_structure(cases, runs, tols, name, arith):
    case, jac = cases[name], runs[(name, arith)]["jac"]
    assert jac.shape == (N, case.E, 6, case.D) and jac.dtype == np.float32
    if name == "iiwa14":
        assert case.D == 7
    if name in ("ref7", "generic5"):
        assert (~case.on_path).any()  # the other wrists, the other branches
    off = np.broadcast_to(~case.on_path[None, :, None, :], jac.shape)
    assert (bits(jac)[off] == 0).all()  # +0.0, bit for bit
    norm = np.linalg.norm(jac[:, :, 3:6].astype(np.float64), axis=2)  # [N, E, D]
    on = np.broadcast_to(case.on_path[None], norm.shape)
    worst = float(np.max(np.abs(norm[on] - 1.0)))
    print(f"{name} {arith}: {int(case.on_path.sum())} of {case.on_path.size} columns on a path; max ||a| - 1| = "
          f"{worst:.3e}, tolerance {tols['ang']:.3e}")
    assert worst <= tols["ang"]


# ------------------------------------------------------------------------------------- 3. positions
@pytest.mark.parametrize("name,arith", params())
def test_positions(cases, runs, tols, name, arith):
    case, r = cases[name], runs[(name, arith)]
    assert r["pos"].shape == (N, case.J, 3)
    d = float(np.max(np.abs(r["pos"].astype(np.float64) - r["epos"].astype(np.float64))))
    d64 = float(np.max(np.abs(r["pos"].astype(np.float64) - case.p64)))
    print(f"{name} {arith}: max |positions - evaluate's| = {d:.3e}, max |positions - float64| = {d64:.3e}, tolerance "
          f"{tols['pos']:.3e}")
    if arith == "reference":
        assert np.array_equal(bits(r["pos"]), bits(r["epos"]))
    else:
        assert d <= tols["pos"]


# ----------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("name,arith", params())
def test_one_vector_alone(runs, name, arith):
    r = runs[(name, arith)]
    assert np.array_equal(bits(r["jac1"]), bits(r["jac"][:1]))
    assert np.array_equal(bits(r["pos1"]), bits(r["pos"][:1]))


# ------------------------------------------------------------------------------------- 5. colliders
@pytest.mark.parametrize("arith", ARITHS)
def test_colliders_change_nothing(cases, runs, tols, arith):
    """A collider changes the build's arithmetic (it may run another sin/cos), not the output: values, not bits."""
    assert np.array_equal(cases["ref7coll"].x, cases["ref7"].x)
    a, b = runs[("ref7coll", arith)], runs[("ref7", arith)]
    e = np.abs(a["jac"].astype(np.float64) - b["jac"].astype(np.float64))
    lin, ang = float(e[:, :, 0:3].max()), float(e[:, :, 3:6].max())
    pos = float(np.max(np.abs(a["pos"].astype(np.float64) - b["pos"].astype(np.float64))))
    print(f"ref7coll against ref7, {arith}: linear {lin:.3e}, angular {ang:.3e}, positions {pos:.3e}")
    assert lin <= tols["lin"] and ang <= tols["ang"] and pos <= tols["pos"]


# ----------------------------------------------------------------------------------- 6. grid stride
def test_grid_stride(cases):
    """More vectors than the grid cap's 8192 x 256 lanes: the last one is a second trip of lane 0."""
    case = cases["generic1"]
    n = 8192 * 256 + 1
    rng = np.random.default_rng(43)
    lo, hi = case.chain["min_rotation"][1].astype(np.float64), case.chain["max_rotation"][1].astype(np.float64)
    x = (lo + rng.uniform(0.0, 1.0, (n, 3)) * (hi - lo)).astype(np.float32)
    x = np.clip(x, lo.astype(np.float32), hi.astype(np.float32))
    pick = np.concatenate([rng.choice(n - 1, 1000, replace=False), [n - 1]])
    s = case.solver("fast")
    sentinel = -12345.0
    xs = dev(x)
    jac = torch.full((n, 1, 6, 3), sentinel, dtype=torch.float32, device="cuda")
    pos = torch.full((n, 1, 3), sentinel, dtype=torch.float32, device="cuda")
    assert s._lib.ikpso_solver_evaluate_jacobian(s._h, xs.data_ptr(), n, pos.data_ptr(), jac.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert bool((jac != sentinel).all()) and bool((pos != sentinel).all())  # every vector was written
    idx = torch.from_numpy(pick).cuda()
    jac, pos = jac[idx].cpu().numpy(), pos[idx].cpu().numpy()
    one_jac = torch.empty((len(pick), 1, 6, 3), dtype=torch.float32, device="cuda")
    one_pos = torch.empty((len(pick), 1, 3), dtype=torch.float32, device="cuda")
    for i, p in enumerate(pick.tolist()):  # each vector alone: lane 0 of one workgroup
        st = s._lib.ikpso_solver_evaluate_jacobian(s._h, xs[p].data_ptr(), 1, one_pos[i].data_ptr(),
                                                   one_jac[i].data_ptr(), None)
        assert st == OK
    torch.cuda.synchronize()
    s.close()
    assert np.array_equal(bits(one_jac.cpu().numpy()), bits(jac))
    assert np.array_equal(bits(one_pos.cpu().numpy()), bits(pos))
    assert np.isfinite(jac).all()


# -------------------------------------------------------------------------------------- 7. statuses
def test_statuses_and_the_empty_call(cases):
    case = cases["ref7"]
    s = case.solver("fast")
    n = 4
    x = dev(case.x[:n])
    sentinel = -12345.0
    jac = torch.full((n, case.E, 6, case.D), sentinel, dtype=torch.float32, device="cuda")
    pos = torch.full((n, case.J, 3), sentinel, dtype=torch.float32, device="cuda")
    fn = s._lib.ikpso_solver_evaluate_jacobian
    assert fn(s._h, x.data_ptr(), 0, pos.data_ptr(), jac.data_ptr(), None) == OK  # no device work ...
    assert fn(s._h, None, 0, None, None, None) == OK
    assert fn(s._h, x.data_ptr(), n, pos.data_ptr(), None, None) == INVALID        # out_jacobian is required
    assert fn(s._h, None, n, pos.data_ptr(), jac.data_ptr(), None) == INVALID
    assert fn(s._h, x.data_ptr(), -1, pos.data_ptr(), jac.data_ptr(), None) == INVALID
    torch.cuda.synchronize()
    assert bool((jac == sentinel).all()) and bool((pos == sentinel).all())         # ... and nothing refused wrote
    assert fn(s._h, x.data_ptr(), n, None, jac.data_ptr(), None) == OK             # out_positions is optional
    torch.cuda.synchronize()
    assert bool((jac != sentinel).all()) and bool((pos == sentinel).all())
    want = jac.cpu().numpy()
    s.close()
    # a cooperative-family solver and a streaming solver are served, by the same build
    for kw in (dict(kernel="coop", P=2048), dict(kernel="streaming")):
        other = case.solver("fast", **kw)
        got, _ = other.jacobian(x)
        other.close()
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), kw
