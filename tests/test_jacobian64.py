"""tests/jacobian64.py, the float64 checker of ikpso_solver_evaluate_jacobian, against central differences of
frames64.node_frames (CPU only).

Step h = 1e-4.  A central difference's truncation term is h^2 / 6 |f'''|.  A node position is a sum of
link vectors, each turned by the angle about an axis through the chain: |p'''| <= reach, the sum of the link
lengths, so the linear rows are held to h^2 reach (a margin of 6); the float64 rounding term eps reach / h
is four orders below it.  A rotation's third derivative along one angle has norm 1, so
vee((dR/dtheta) R^T) is held to h^2.  Columns off an effector's path are exactly 0."""
import numpy as np
import pytest

import frames64
import ikpso
import jacobian64
import topologies as tp
from ikpso.dh import iiwa14

H = 1e-4
POSES = 16


def _chains():
    arm = iiwa14()
    return {
        "ref7": (ikpso.reference_scene(reset=True).origin.to_cuda(), None),
        "serial6": (tp.serial(6), None),
        "generic5": (tp.random_tree(5, 0), None),
        "generic1": (tp.random_tree(1, 0), None),
        "serial20": (tp.serial(20), None),
        "iiwa14": (arm.origin.to_cuda(), arm.axis_mask),
    }


CHAINS = _chains()


def vee(S):
    """The vector of the skew part of [..., 3, 3]."""
    return np.stack([S[..., 2, 1] - S[..., 1, 2], S[..., 0, 2] - S[..., 2, 0], S[..., 1, 0] - S[..., 0, 1]], axis=-1) / 2.0


@pytest.mark.parametrize("name", list(CHAINS))
def test_checker_against_central_differences(name):
    chain, mask = CHAINS[name]
    rng = np.random.default_rng([7, len(chain)])
    x = tp.random_poses(chain, POSES, rng, mask)
    free, eff = tp.free_axes(chain, mask), tp.effectors(chain)
    jac = jacobian64.effector_jacobian(chain, x, mask)
    assert jac.shape == (POSES, len(eff), 6, len(free)) and jac.dtype == np.float64
    full = tp.expand(chain, x, mask).astype(np.float64)
    _, R = frames64.node_frames(chain, full)
    reach = float(np.sum(np.abs(chain["length"][1:].astype(np.float64))))
    worst_lin = worst_ang = 0.0
    for d, (k, c) in enumerate(free):
        step = np.zeros_like(full)
        step[:, 3 * (k - 1) + c] = H
        pp, Rp = frames64.node_frames(chain, full + step)
        pm, Rm = frames64.node_frames(chain, full - step)
        dp, dR = (pp - pm) / (2.0 * H), (Rp - Rm) / (2.0 * H)
        for e, m in enumerate(eff):
            lin, ang = dp[:, m - 1], vee(dR[:, m - 1] @ np.swapaxes(R[:, m - 1], -1, -2))
            if k in jacobian64.ancestors(chain, int(m)):
                worst_lin = max(worst_lin, float(np.max(np.abs(jac[:, e, 0:3, d] - lin))))
                worst_ang = max(worst_ang, float(np.max(np.abs(jac[:, e, 3:6, d] - ang))))
                assert np.allclose(np.linalg.norm(jac[:, e, 3:6, d], axis=-1), 1.0, rtol=0, atol=1e-12)
            else:
                assert np.array_equal(jac[:, e, :, d], np.zeros((POSES, 6)))
                assert np.array_equal(lin, np.zeros((POSES, 3))) and np.array_equal(dR[:, m - 1], np.zeros((POSES, 3, 3)))
    print(f"{name}: D={len(free)} E={len(eff)} reach {reach:.3f}: max |linear - difference| = {worst_lin:.3e} "
          f"(bound {H * H * reach:.3e}), max |angular - difference| = {worst_ang:.3e} (bound {H * H:.3e})")
    assert worst_lin <= H * H * reach
    assert worst_ang <= H * H


def test_float32_restatement_is_close():
    """The dtype parameter restates the same expressions: float32 differs by rounding alone."""
    chain, mask = CHAINS["ref7"]
    x = tp.random_poses(chain, POSES, np.random.default_rng(3), mask)
    j64 = jacobian64.effector_jacobian(chain, x, mask)
    j32 = jacobian64.effector_jacobian(chain, x, mask, dtype=np.float32)
    assert j32.dtype == np.float32 and j32.shape == j64.shape
    assert 0.0 < float(np.max(np.abs(j32.astype(np.float64) - j64))) < 1e-5
    assert np.array_equal(j32 == 0, j64 == 0)


def test_manipulability():
    """sqrt(det(J J^T)) over the chosen rows: a planar two-link arm's is l1 l2 |sin q2|."""
    l1, l2, q1, q2 = 0.7, 0.4, 0.3, 1.1
    s1, c1, s12, c12 = np.sin(q1), np.cos(q1), np.sin(q1 + q2), np.cos(q1 + q2)
    J = np.zeros((6, 2))
    J[0] = [-l1 * s1 - l2 * s12, -l2 * s12]
    J[1] = [l1 * c1 + l2 * c12, l2 * c12]
    J[5] = [1.0, 1.0]
    assert abs(float(ikpso.manipulability(J, rows=slice(0, 2))) - l1 * l2 * abs(np.sin(q2))) < 1e-12
    assert float(ikpso.manipulability(J)) == 0.0  # three linear rows of a planar arm: singular
    chain, mask = CHAINS["iiwa14"]
    jac = jacobian64.effector_jacobian(chain, tp.random_poses(chain, POSES, np.random.default_rng(5), mask), mask)
    w = ikpso.manipulability(jac)
    assert w.shape == (POSES, 1) and w.dtype == np.float64 and (w > 0).all()
    want = np.sqrt(np.linalg.det(jac[:, 0, :6] @ np.swapaxes(jac[:, 0, :6], -1, -2)))
    assert np.allclose(ikpso.manipulability(jac, rows=slice(0, 6))[:, 0], want, rtol=1e-12, atol=0)
