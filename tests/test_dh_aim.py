"""DHArm.node_axis on the CPU, float64: an axis named in the textbook DH tool frame, carried into the
effector node's frame, points where the textbook tool frame points it.

The effector node's frame is pose64.effector_frames over Euler vectors rebuilt in float64 from the
DH parameters by the mapping ikpso.dh documents (as tests/test_dh_pose.py rebuilds them): the node
table itself holds float32, whose +-pi/2 are 4e-8 off -- too coarse for a 1e-9 statement (1.4e-7 seen).
"""
import numpy as np

import pose64
import topologies as tp
from ikpso.dh import IIWA14, dh_forward_pose, euler_xyz, iiwa14


def euler64(arm, chain, theta) -> np.ndarray:
    """[n, 3 J] float64 Euler vectors of the arm's nodes at joint angles theta [n, joints]."""
    a, alpha, d = IIWA14["a"], IIWA14["alpha"], IIWA14["d"]
    cols, k = [], np.eye(3)
    for i in range(len(a)):
        x, y, z = euler_xyz(k)
        cols += [np.full(len(theta), x), np.full(len(theta), y), z + theta[:, i]]
        if float(d[i]) != 0.0:
            beta = float(np.arctan2(-float(d[i]), float(a[i])))
            cols += [np.zeros(len(theta)), np.full(len(theta), beta), np.zeros(len(theta))]
            k = tp._rot(1, np.array(-beta)) @ tp._rot(0, np.array(float(alpha[i])))
        else:
            k = tp._rot(0, np.array(float(alpha[i])))
    full = np.stack(cols, axis=1)
    assert full.shape[1] == 3 * (len(chain) - 1)
    return full


def test_node_axis_points_where_the_tool_axis_points():
    arm = iiwa14()
    chain, mask = arm.origin.to_cuda(), arm.axis_mask
    rng = np.random.default_rng(5)
    free = tp.random_poses(chain, 16, rng, mask)
    theta = np.array([arm.joint_angles(x) for x in free])
    full = euler64(arm, chain, theta)
    assert np.allclose(full, tp.expand(chain, free, mask), atol=1e-6)  # the node table, to float32 rounding
    frames = pose64.effector_frames(chain, full)
    for a_tool in ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)):
        a_node = arm.node_axis(a_tool)
        assert a_node.shape == (3,) and a_node.dtype == np.float64
        assert abs(np.linalg.norm(a_node) - 1.0) <= 1e-12
        worst = 0.0
        for t, f in zip(theta, frames):
            want = dh_forward_pose(t, IIWA14["d"], IIWA14["a"], IIWA14["alpha"])[:3, :3] @ np.asarray(a_tool)
            worst = max(worst, float(np.max(np.abs(f @ a_node - want))))
        print(f"axis {np.asarray(a_tool).tolist()}: max |R_node node_axis(a) - R_tool a| = {worst:.3e}")
        assert worst <= 1e-9
