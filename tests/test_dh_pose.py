"""ikpso.dh's pose side on the CPU, float64: dh_forward_pose against dh_forward, and the constant
DHArm.tool_rotation between the effector node's frame (the Euler definition over the node table)
and the textbook DH tool frame."""
import numpy as np
import pytest

import topologies as tp
from ikpso.dh import IIWA14, dh_forward, dh_forward_pose, euler_xyz, iiwa14


def arms():
    arm6, a, alpha, d = tp.dh_arm_n(6)
    return [("iiwa14", iiwa14(), IIWA14["a"], IIWA14["alpha"], IIWA14["d"]), ("dh_arm_n(6)", arm6, a, alpha, d)]


def node_angles64(arm, a, alpha, d):
    """The Euler angles of the arm's nodes in float64, [(x, y, z, joint index or None)], rebuilt from
    the DH parameters by the mapping ikpso.dh documents -- the node table itself holds float32, too
    coarse for a 1e-12 statement -- and checked against that table to float32 rounding."""
    rows, k = [], np.eye(3)
    for i in range(len(a)):
        rows.append((*euler_xyz(k), i))
        if float(d[i]) != 0.0:
            beta = float(np.arctan2(-float(d[i]), float(a[i])))
            rows.append((0.0, beta, 0.0, None))
            k = tp._rot(1, np.array(-beta)) @ tp._rot(0, np.array(float(alpha[i])))
        else:
            k = tp._rot(0, np.array(float(alpha[i])))
    nodes = list(arm.origin.dfs())[1:]
    assert len(nodes) == len(rows)
    for n, (x, y, z, j) in zip(nodes, rows):
        assert np.allclose(np.asarray(n.rotation, dtype=np.float64), (x, y, z), atol=1e-6)
        assert (j is not None) == any(n is jn for jn in arm.joint_nodes)
    assert not np.asarray(arm.origin.rotation).any()
    return rows


def node_frames(arm, a, alpha, d, theta) -> np.ndarray:
    """[n, 3, 3] float64: world rotation of the tool node's frame at joint angles theta [n, joints]
    by the Euler definition: Rx Ry Rz of every node from the (unturned) origin down."""
    R = np.broadcast_to(np.eye(3), (len(theta), 3, 3))
    for x, y, z, j in node_angles64(arm, a, alpha, d):
        zz = np.full(len(theta), z) if j is None else z + theta[:, j]
        R = R @ tp._rot(0, np.full(len(theta), x)) @ tp._rot(1, np.full(len(theta), y)) @ tp._rot(2, zz)
    return R


@pytest.mark.parametrize("case", arms(), ids=lambda c: c[0])
def test_pose_translation_is_dh_forward(case):
    _, arm, a, alpha, d = case
    rng = np.random.default_rng(3)
    for theta in rng.uniform(-2.0, 2.0, (8, arm.joints)):
        m = dh_forward_pose(theta, d, a, alpha)
        assert m.shape == (4, 4) and m.dtype == np.float64
        assert np.array_equal(m[:3, 3], dh_forward(theta, d, a, alpha))
        assert np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0])


@pytest.mark.parametrize("case", arms(), ids=lambda c: c[0])
def test_effector_frame_times_tool_rotation_is_the_textbook_rotation(case):
    _, arm, a, alpha, d = case
    rng = np.random.default_rng(4)
    theta = rng.uniform(-2.0, 2.0, (8, arm.joints))
    K = arm.tool_rotation
    assert K.shape == (3, 3) and np.allclose(K @ K.T, np.eye(3), atol=1e-15)
    frames = node_frames(arm, a, alpha, d, theta)
    for t, f in zip(theta, frames):
        want = dh_forward_pose(t, d, a, alpha)[:3, :3]
        assert np.max(np.abs(f @ K - want)) <= 1e-12
        assert np.max(np.abs(arm.node_target(want) - f)) <= 1e-12
