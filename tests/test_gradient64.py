"""tests/gradient64.py, the float64 checker of ikpso_solver_evaluate_gradient, held to three things (CPU only):
central differences of its own fitness64, the fitness of tests/frames64.py and of the CPU oracle, and
tests/jacobian64.py's Jacobians contracted with the residuals.

Central differences, step h = 1e-4: the truncation term is h^2 / 6 |f'''| along one angle.  With reach the sum
of the link lengths (every |p'|, |p''|, |p'''| along one angle is at most reach) and r a bound on |p - t|
(reach plus the farthest target from the origin),
    |d^3/dtheta^3 w |p - t|^2|   = 2 w |(p - t) . p''' + 3 p' . p''|  <= w (2 r reach + 6 reach^2)
    |d^3/dtheta^3 w rw |R - T|^2| = 2 w rw |tr(T^T R''')|              <= 2 sqrt(2) w rw |T|_F
(R''' = [a]x^3 R has Frobenius norm sqrt(2)); the angle term is quadratic.  The case's scale S is the sum of
these bounds over every effector and, with the distance term, every node; a gradient entry is held to h^2 S (a
margin of 6; float64 rounding, eps f / h, is orders below).  The soft-limit penalty is C1 only: its second
derivative jumps by 2 limit_weight at a soft bound, so a central difference that straddles a bound (|x - bound|
< h) is off by up to limit_weight h / 2; those entries, and only those, get limit_weight h added."""
import numpy as np
import pytest

import frames64
import gradient64
import ikpso
import jacobian64
import topologies as tp
from gradient64 import Terms
from ikpso.dh import iiwa14

H = 1e-4
POSES = 16
NAMES = ("ref7", "serial6", "serial20", "generic5", "generic1", "iiwa14")
VARIANTS = ("plain", "distance", "distance_node_slot", "penalty", "rotation", "rotation_skew", "all")


def chain_of(name):
    if name == "ref7":
        return ikpso.reference_scene(reset=True).origin.to_cuda(), None
    if name == "iiwa14":
        arm = iiwa14()
        return arm.origin.to_cuda(), arm.axis_mask
    J = int(name.lstrip("abcdefghijklmnopqrstuvwxyz"))
    return (tp.serial(J) if name.startswith("serial") else tp.random_tree(J, 0)), None


def soft_limits(chain, mask, shrink=0.25):
    """Soft bounds a quarter of the clamp range inside each clamp bound: about half of uniformly drawn
    in-bounds angles lie beyond one of them."""
    free = tp.free_axes(chain, mask)
    lo = np.array([chain["min_rotation"][k][c] for k, c in free], dtype=np.float64)
    hi = np.array([chain["max_rotation"][k][c] for k, c in free], dtype=np.float64)
    return (lo + shrink * (hi - lo)).astype(np.float32), (hi - shrink * (hi - lo)).astype(np.float32)


def reference_positions(chain, rng):
    """A [4 (J + 2)] positions array: every slot a point within the reach and a w in [0, 1]."""
    J = len(chain) - 1
    reach = float(np.sum(np.abs(chain["length"][1:])))
    p = np.concatenate([rng.uniform(-reach, reach, (J + 2, 3)), rng.uniform(0.0, 1.0, (J + 2, 1))], axis=1)
    return p.astype(np.float32).reshape(-1)


def make_case(name, variant, n=POSES, seed=7):
    """(chain, mask, x, rest, targets, terms, target_rot, rot_weights) of one case."""
    chain, mask = chain_of(name)
    rng = np.random.default_rng([seed, len(chain), VARIANTS.index(variant)])
    x, rest, other = (tp.random_poses(chain, n, rng, mask) for _ in range(3))
    p, R = frames64.effector_frames(chain, other, mask)
    targets, trot, rw = p.astype(np.float32), None, None
    terms = Terms()
    if variant in ("distance", "distance_node_slot", "all"):
        terms.distance_weight, terms.positions = 1.5, reference_positions(chain, rng)
        terms.node_slot = variant != "distance"
    if variant in ("penalty", "all"):
        terms.limit_weight = 2.0
        terms.soft_lo, terms.soft_hi = soft_limits(chain, mask)
    if variant in ("rotation", "rotation_skew", "all"):
        trot = R.astype(np.float32)
        if variant == "rotation_skew":  # used as given: not orthonormal
            trot = (trot * 1.3 + rng.uniform(-0.4, 0.4, trot.shape)).astype(np.float32)
        rw = np.array([(1.0, 0.0, 0.5)[e % 3] for e in range(len(p[0]))], np.float32)
        if len(rw) == 1:
            rw[:] = 0.75
    return chain, mask, x, rest, targets, terms, trot, rw


def third_derivative_scale(chain, targets, terms, trot, rw):
    J = len(chain) - 1
    reach = float(np.sum(np.abs(chain["length"][1:].astype(np.float64))))
    o = chain["position"][0].astype(np.float64)
    eff = tp.effectors(chain)
    w = chain["effector_weight"][eff].astype(np.float64)
    S = 0.0
    for e in range(len(eff)):
        r = reach + float(np.max(np.linalg.norm(targets[:, e].astype(np.float64) - o, axis=1)))
        S += w[e] * (2.0 * r * reach + 6.0 * reach * reach)
        if rw is not None and rw[e] != 0:
            S += 2.0 * np.sqrt(2.0) * w[e] * float(rw[e]) * float(np.max(np.linalg.norm(trot[:, e].astype(np.float64), axis=(1, 2))))
    refs = terms.refs(J, np.float64)
    if refs is not None:
        for k in range(J):
            r = reach + float(np.linalg.norm(refs[0][k] - o))
            S += terms.distance_weight / J * (2.0 * r * reach + 6.0 * reach * reach)
    return S


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", NAMES)
def test_checker_against_central_differences(name, variant):
    chain, mask, x, rest, targets, terms, trot, rw = make_case(name, variant)
    g = gradient64.gradient64(chain, x, rest, targets, terms, trot, rw, mask)
    D = len(tp.free_axes(chain, mask))
    assert g.shape == (POSES, D) and g.dtype == np.float64
    S = third_derivative_scale(chain, targets, terms, trot, rw)
    xd = x.astype(np.float64)

    def f(v):  # fitness64 takes float32 angle vectors; the differences need float64 ones
        return _fitness_at(chain, v, rest, targets, terms, trot, rw, mask)

    worst = worst_kink = 0.0
    beyond = 0
    for d in range(D):
        step = np.zeros_like(xd)
        step[:, d] = H
        diff = (f(xd + step) - f(xd - step)) / (2.0 * H)
        err = np.abs(g[:, d] - diff)
        kink = np.zeros(POSES, dtype=bool)
        if terms.penalised():
            kink = (np.abs(xd[:, d] - terms.soft_lo[d]) < H) | (np.abs(xd[:, d] - terms.soft_hi[d]) < H)
            beyond += int(np.sum((xd[:, d] > terms.soft_hi[d]) | (xd[:, d] < terms.soft_lo[d])))
        bound = H * H * S + np.where(kink, terms.limit_weight * H, 0.0)
        worst = max(worst, float(err[~kink].max(initial=0.0)))
        worst_kink = max(worst_kink, float(err[kink].max(initial=0.0)))
        assert (err <= bound).all(), (d, float(err.max()), H * H * S)
    print(f"{name} {variant}: D={D} scale S={S:.3e}: max |gradient64 - difference| = {worst:.3e} (bound {H * H * S:.3e})"
          + (f"; {beyond} of {POSES * D} angles beyond a soft bound, straddling entries worst {worst_kink:.3e}"
             if terms.penalised() else ""))
    if terms.penalised():
        assert beyond >= POSES * D // 4  # a good share of the angles lie beyond the soft limits


def _fitness_at(chain, v64, rest, targets, terms, trot, rw, mask):
    """fitness64 at float64 angle vectors (gradient64's own fitness rounds its angles to float32 first, as
    the entry's are): the same expressions on frames64.node_frames of the float64 vectors."""
    full = tp.expand(chain, np.zeros(v64.shape, np.float32), mask).astype(np.float64)
    full[:, [3 * (k - 1) + c for k, c in tp.free_axes(chain, mask)]] = v64
    n, J = len(full), len(chain) - 1
    p, R = frames64.node_frames(chain, full)
    eff = tp.effectors(chain)
    w = chain["effector_weight"][eff].astype(np.float64)
    f = np.zeros(n)
    for e, m in enumerate(eff):
        f += w[e] * np.sum((p[:, m - 1] - targets[:, e].astype(np.float64)) ** 2, axis=1)
        if rw is not None and rw[e] != 0:
            f += w[e] * float(rw[e]) * np.sum((R[:, m - 1] - trot[:, e].astype(np.float64)) ** 2, axis=(1, 2))
    refs = terms.refs(J, np.float64)
    if refs is not None:
        f += terms.distance_weight / J * (np.sum((p - refs[0][None]) ** 2, axis=(1, 2)) + np.sum((1.0 - refs[1]) ** 2))
    f += terms.angle_weight / J * np.sum((rest.astype(np.float64) - v64) ** 2, axis=1)
    if terms.penalised():
        over = np.maximum(np.maximum(v64 - terms.soft_hi.astype(np.float64), terms.soft_lo.astype(np.float64) - v64), 0.0)
        f += terms.limit_weight * np.sum(over ** 2, axis=1)
    return f


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ("ref7", "generic5", "iiwa14"))
def test_fitness64_is_the_differenced_fitness(name, variant):
    """The float64-angle restatement the differences run on is fitness64 at the float32 vectors."""
    chain, mask, x, rest, targets, terms, trot, rw = make_case(name, variant)
    a = gradient64.fitness64(chain, x, rest, targets, terms, trot, rw, mask)
    b = _fitness_at(chain, x.astype(np.float64), rest, targets, terms, trot, rw, mask)
    assert np.allclose(a, b, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", NAMES)
def test_fitness64_against_frames64(name):
    """Where the terms coincide (positions, angle term, rotation term): tests/frames64.py's fitness."""
    chain, mask, x, rest, targets, terms, trot, rw = make_case(name, "rotation")
    want = frames64.frames_fitness(chain, terms.angle_weight, x, rest, targets, trot, rw, mask)
    assert np.allclose(gradient64.fitness64(chain, x, rest, targets, terms, trot, rw, mask), want, rtol=1e-12, atol=0)
    zero = frames64.frames_fitness(chain, terms.angle_weight, x, rest, targets, trot, np.zeros_like(rw), mask)
    assert np.allclose(gradient64.fitness64(chain, x, rest, targets, terms, mask=mask), zero, rtol=1e-12, atol=0)


@pytest.mark.parametrize("variant", ("plain", "distance", "distance_node_slot", "penalty"))
@pytest.mark.parametrize("name", ("ref7", "generic5"))
def test_fitness64_against_the_oracle(oracle, name, variant):
    """Where the oracle has the term (its own targets and rest rotation): within four times the float32
    restatement's spread plus the relative rounding of a float32 sum of this many terms."""
    chain, mask, x, _, _, terms, _, _ = make_case(name, variant)
    eff = tp.effectors(chain)
    rest = np.repeat(np.asarray(chain["rotation"][1:], np.float32).reshape(1, -1), POSES, axis=0)
    targets = np.repeat(chain["target_position"][eff].astype(np.float32)[None], POSES, axis=0)
    got = gradient64.fitness64(chain, x, rest, targets, terms)
    got32 = gradient64.fitness64(chain, x, rest, targets, terms, dtype=np.float32).astype(np.float64)
    positions = None if terms.positions is None else (terms.positions[8:] if terms.node_slot else terms.positions)
    want = np.array([oracle.fitness(chain, v, terms.angle_weight, terms.distance_weight, positions, terms.limit_weight,
                                    terms.soft_lo, terms.soft_hi) for v in x], dtype=np.float64)
    tol = 4.0 * float(np.max(np.abs(got32 - got)))
    print(f"{name} {variant}: fitness {got.min():.3e}..{got.max():.3e}, max |fitness64 - oracle| = "
          f"{np.max(np.abs(got - want)):.3e}, tolerance {tol:.3e}")
    assert tol > 0 and (np.abs(got - want) <= tol).all()


@pytest.mark.parametrize("name", NAMES)
def test_position_and_rotation_parts_against_the_jacobian(name):
    """sum_e 2 w_e (p_e - t_e) . J_lin[e] and sum_e 2 w_e rw_e v(R_e T_e^T) . J_ang[e]."""
    chain, mask, x, rest, targets, terms, trot, rw = make_case(name, "rotation")
    parts = gradient64.gradient64(chain, x, rest, targets, terms, trot, rw, mask, parts=True)
    jac = jacobian64.effector_jacobian(chain, x, mask)
    p, R = frames64.effector_frames(chain, x, mask)
    w = chain["effector_weight"][tp.effectors(chain)].astype(np.float64)
    res = 2.0 * w[None, :, None] * (p - targets.astype(np.float64))
    pos = np.einsum("nei,neid->nd", res, jac[:, :, 0:3])
    M = R @ np.swapaxes(trot.astype(np.float64), -1, -2)
    v = np.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], axis=-1)
    rot = np.einsum("nei,neid->nd", 2.0 * (w * rw.astype(np.float64))[None, :, None] * v, jac[:, :, 3:6])
    scale = max(1.0, float(np.max(np.abs(pos))), float(np.max(np.abs(rot))))
    assert float(np.max(np.abs(parts["position"] - pos))) <= 1e-12 * scale
    assert float(np.max(np.abs(parts["rotation"] - rot))) <= 1e-12 * scale
    assert not parts["distance"].any() and not parts["penalty"].any()
    assert np.array_equal(parts["angle"], 2.0 * (terms.angle_weight / (len(chain) - 1)) * (x.astype(np.float64) - rest))


def test_float32_restatement_is_close():
    chain, mask, x, rest, targets, terms, trot, rw = make_case("ref7", "all")
    g64 = gradient64.gradient64(chain, x, rest, targets, terms, trot, rw, mask)
    g32 = gradient64.gradient64(chain, x, rest, targets, terms, trot, rw, mask, dtype=np.float32)
    assert g32.dtype == np.float32 and g32.shape == g64.shape
    assert 0.0 < float(np.max(np.abs(g32.astype(np.float64) - g64))) < 1e-4
