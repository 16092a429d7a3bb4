"""World frames of every effector of a tree and the fitness of ikpso_solve_track_frames in numpy
float64, from the node table and the definitions alone (include/ikpso.h).  Test
infrastructure, imported like tests/topologies.py and tests/pose64.py; nothing here touches a GPU or
the library.  `dtype` restates the same expressions in another precision (np.float32: what a valid
fp32 evaluation of them may differ by)."""
import numpy as np

import topologies as tp


def _rot(axis: int, a: np.ndarray, dtype) -> np.ndarray:
    """[n, 3, 3] rotations about x, y or z by the angles a [n], in dtype."""
    a = np.asarray(a, dtype=dtype)
    c, s = np.cos(a), np.sin(a)
    m = np.zeros(a.shape + (3, 3), dtype=dtype)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[..., axis, axis] = 1.0
    m[..., i, i] = c
    m[..., j, j] = c
    m[..., i, j] = -s
    m[..., j, i] = s
    return m


def node_frames(chain, full_euler_angles, dtype=np.float64):
    """(positions [n, J, 3], rotations [n, J, 3, 3]) of nodes 1..J for full Euler vectors [n, 3 J]:
    frame(0) = T(origin position) Rx Ry Rz(origin rotation); frame(k) = frame(parent(k)) Rx(x_k)
    Ry(y_k) Rz(z_k) T(length_k, 0, 0).  A node's rotation is its frame's (the link's translation turns
    nothing), its position the frame's translation."""
    ang = np.asarray(full_euler_angles, dtype=dtype)
    ang = ang.reshape(len(ang), -1, 3)
    n, J = ang.shape[0], len(chain) - 1
    assert ang.shape[1] == J
    o = np.asarray(chain["rotation"][0], dtype=dtype)
    R, p = [None] * (J + 1), [None] * (J + 1)
    R[0] = np.broadcast_to(_rot(0, o[0:1], dtype) @ _rot(1, o[1:2], dtype) @ _rot(2, o[2:3], dtype), (n, 3, 3))
    p[0] = np.broadcast_to(np.asarray(chain["position"][0], dtype=dtype), (n, 3))
    for k in range(1, J + 1):
        par = int(chain["parent_index"][k])
        R[k] = R[par] @ _rot(0, ang[:, k - 1, 0], dtype) @ _rot(1, ang[:, k - 1, 1], dtype) @ _rot(2, ang[:, k - 1, 2], dtype)
        p[k] = p[par] + dtype(chain["length"][k]) * R[k][:, :, 0]
    return np.stack(p[1:], axis=1), np.stack(R[1:], axis=1)


def effector_frames(chain, free_angles, mask=None, dtype=np.float64):
    """(positions [n, E, 3], rotations [n, E, 3, 3]) of the effectors, in node order, for free-axis
    vectors [n, D] (locked axes at the chain's rotation)."""
    full = tp.expand(chain, np.asarray(free_angles, dtype=np.float32), mask)
    p, R = node_frames(chain, full, dtype)
    e = tp.effectors(chain) - 1
    return p[:, e], R[:, e]


def geodesic(Ra, Rb) -> np.ndarray:
    """Angle between rotations [..., 3, 3], from the chord |Ra - Rb|_F = 2 sqrt(2) sin(theta / 2)."""
    chord = np.linalg.norm(np.asarray(Ra, np.float64) - np.asarray(Rb, np.float64), axis=(-2, -1))
    return 2.0 * np.arcsin(np.clip(chord / (2.0 * np.sqrt(2.0)), 0.0, 1.0))


def frames_fitness(chain, angle_weight, answers, rest, targets, target_rot, rot_weights, mask=None,
                   dtype=np.float64) -> np.ndarray:
    """[n] fitness of free-axis answers [n, D] as the header states it: ikpso_solve_track's
    sum_e w_e |p_e - t_e|^2 + (angle_weight / J) sum (rest - x)^2 (rest [n, D]: the frame's start
    pose; no distance, penalty or collider term), plus, accumulated over the effectors in node
    order and added last, sum_e w_e rot_weights[e] |R_e - target_rot[e]|_F^2.  targets [n, E, 3],
    target_rot [n, E, 3, 3], rot_weights [E]."""
    J = len(chain) - 1
    eff = tp.effectors(chain)
    w = np.asarray(chain["effector_weight"][eff], dtype=dtype)
    rw = np.asarray(rot_weights, dtype=dtype).reshape(len(eff))
    p, R = effector_frames(chain, answers, mask, dtype)
    n = len(p)
    t = np.asarray(targets, dtype=dtype).reshape(n, len(eff), 3)
    Rt = np.asarray(target_rot, dtype=dtype).reshape(n, len(eff), 3, 3)
    x, r = np.asarray(answers, dtype=dtype), np.asarray(rest, dtype=dtype)
    position, orient = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    for e in range(len(eff)):
        position = position + np.sum((p[:, e] - t[:, e]) ** 2, axis=1, dtype=dtype) * w[e]
        if rw[e] != 0:  # a weight of 0 leaves the effector position-only
            orient = orient + (w[e] * rw[e]) * np.sum((R[:, e] - Rt[:, e]) ** 2, axis=(1, 2), dtype=dtype)
    angle = dtype(dtype(angle_weight) / dtype(J)) * np.sum((r - x) ** 2, axis=1, dtype=dtype)
    return (position + angle) + orient
