"""The geometric Jacobian of every effector of a tree in numpy float64, from the node table and the
definition alone (include/ikpso.h, ikpso_solver_evaluate_jacobian), on top of frames64.node_frames.  Test
infrastructure, imported like tests/frames64.py; nothing here touches a GPU or the library.  `dtype`
restates the same expressions in another precision (np.float32: what a valid fp32 evaluation of them may
differ by)."""
import numpy as np

import frames64
import topologies as tp


def ancestors(chain, m: int) -> list:
    """Node m and its ancestors below the origin, m first."""
    out = []
    while m > 0:
        out.append(m)
        m = int(chain["parent_index"][m])
    return out


def effector_jacobian(chain, free_angles, mask=None, dtype=np.float64) -> np.ndarray:
    """[n, E, 6, D] for free-axis vectors [n, D] (locked axes at the chain's rotation): effectors in node
    order, rows 0..2 linear and 3..5 angular, world coordinates, one column per free axis in
    tp.free_axes' order.  For effector node m and the angle c of node k, k = m or an ancestor of m, the
    column is (a x (p_m - p_parent(k)), a) with the world axis
        c = 0: a = R_parent(k) e_x,   c = 1: a = R_parent(k) Rx(x_k) e_y,   c = 2: a = R_k e_z;
    every other column is 0."""
    full = tp.expand(chain, np.asarray(free_angles, dtype=np.float32), mask)
    n, J = len(full), len(chain) - 1
    p, R = frames64.node_frames(chain, full, dtype)
    ang = np.asarray(full, dtype=dtype).reshape(n, J, 3)
    o = np.asarray(chain["rotation"][0], dtype=dtype)
    R0 = frames64._rot(0, o[0:1], dtype) @ frames64._rot(1, o[1:2], dtype) @ frames64._rot(2, o[2:3], dtype)
    Rn = [np.broadcast_to(R0, (n, 3, 3))] + [R[:, k] for k in range(J)]                       # by node index
    pn = [np.broadcast_to(np.asarray(chain["position"][0], dtype=dtype), (n, 3))] + [p[:, k] for k in range(J)]
    free, eff = tp.free_axes(chain, mask), tp.effectors(chain)
    jac = np.zeros((n, len(eff), 6, len(free)), dtype=dtype)
    for e, m in enumerate(eff):
        path = ancestors(chain, int(m))
        for d, (k, c) in enumerate(free):
            if k not in path:
                continue
            par = int(chain["parent_index"][k])
            if c == 0:
                a = Rn[par][:, :, 0]
            elif c == 1:
                a = (Rn[par] @ frames64._rot(0, ang[:, k - 1, 0], dtype))[:, :, 1]
            else:
                a = Rn[k][:, :, 2]
            jac[:, e, 0:3, d] = np.cross(a, pn[int(m)] - pn[par]).astype(dtype)
            jac[:, e, 3:6, d] = a
    return jac
