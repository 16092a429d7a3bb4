"""The effector node's frame and the pose fitness in numpy float64, from the node table and the
definitions alone (include/ikpso.h: ikpso_solve_track_pose).  Test infrastructure,
imported like tests/topologies.py; nothing here touches a GPU or the library."""
import numpy as np

import topologies as tp


def effector_frames(chain, full_euler_angles) -> np.ndarray:
    """[n, 3, 3]: world rotation of the LAST node's frame of a serial chain for full Euler vectors
    [n, 3 J]: the origin's Rx Ry Rz, then Rx Ry Rz of every node (a link's translation turns nothing)."""
    ang = np.asarray(full_euler_angles, dtype=np.float64)
    ang = ang.reshape(len(ang), -1, 3)
    assert tp.is_serial_tip(chain) and ang.shape[1] == len(chain) - 1
    o = np.asarray(chain["rotation"][0], dtype=np.float64)
    R = np.broadcast_to(tp._rot(0, o[0:1]) @ tp._rot(1, o[1:2]) @ tp._rot(2, o[2:3]), (len(ang), 3, 3))
    for k in range(ang.shape[1]):
        R = R @ tp._rot(0, ang[:, k, 0]) @ tp._rot(1, ang[:, k, 1]) @ tp._rot(2, ang[:, k, 2])
    return R


def poses(chain, free_angles, mask):
    """(tip positions [n, 3], effector frames [n, 3, 3]) of free-axis vectors [n, D], float64."""
    full = tp.expand(chain, np.asarray(free_angles, dtype=np.float32), mask)
    return tp.fk64(chain, full)[:, -1, :], effector_frames(chain, full)


def geodesic(Ra, Rb) -> np.ndarray:
    """[n] angle between rotations [n, 3, 3], from the chord |Ra - Rb|_F = 2 sqrt(2) sin(theta / 2)
    (well conditioned at small angles, where the trace form is not)."""
    chord = np.linalg.norm(np.asarray(Ra, np.float64) - np.asarray(Rb, np.float64), axis=(-2, -1))
    return 2.0 * np.arcsin(np.clip(chord / (2.0 * np.sqrt(2.0)), 0.0, 1.0))


def pose_fitness(chain, mask, angle_weight, answers, rest, targets, target_rot, orientation_weight) -> np.ndarray:
    """[n] float64 fitness of free-axis answers [n, D] as the header states it: the tip term
    w_e |p - t|^2, the angle term (angle_weight / J) sum (rest - x)^2 over the free axes (the locked
    ones add zeros) with rest [n, D] the frame's start pose, and the orientation term
    w_e * orientation_weight * |R_eff - R_target|_F^2.  No penalty, distance or collider term."""
    J = len(chain) - 1
    w_e = float(chain["effector_weight"][J])
    p, R = poses(chain, answers, mask)
    t = np.asarray(targets, dtype=np.float64).reshape(len(p), 3)
    Rt = np.asarray(target_rot, dtype=np.float64).reshape(len(p), 3, 3)
    x, r = np.asarray(answers, dtype=np.float64), np.asarray(rest, dtype=np.float64)
    position = w_e * np.sum((p - t) ** 2, axis=1)
    angle = (float(angle_weight) / J) * np.sum((r - x) ** 2, axis=1)
    orient = w_e * float(orientation_weight) * np.sum((R - Rt) ** 2, axis=(1, 2))
    return position + angle + orient
