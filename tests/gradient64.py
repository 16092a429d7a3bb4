"""The fitness ikpso_solver_evaluate_gradient reports (without the collider term) and its gradient in numpy
float64, from the node table and the header's definition alone (include/ikpso.h), on top of
frames64.node_frames.  Test infrastructure, imported like tests/jacobian64.py; nothing here touches a GPU or
the library.  The gradient is assembled pair by pair -- every (free dimension, node below it) on its own,
from the node frames -- which is on purpose not the kernel's route (one reverse sweep carrying a wrench).
`dtype` restates the same expressions in another precision (np.float32: what a valid fp32 evaluation of them
may differ by)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import frames64
import jacobian64
import topologies as tp


@dataclass
class Terms:
    """The objective's configuration beside the chain: BatchSolver's arguments of the same names.  positions is
    the [4 (J + 2)] array of the distance term (read at slot k - 1 for node k, or at slot k + 1 with
    node_slot, IKPSO_FLAG_POSREF_NODE_SLOT); soft_lo / soft_hi are per free dimension."""
    angle_weight: float = 3.0
    distance_weight: float = 0.0
    positions: Optional[np.ndarray] = None
    node_slot: bool = False
    limit_weight: float = 0.0
    soft_lo: Optional[np.ndarray] = None
    soft_hi: Optional[np.ndarray] = None

    def refs(self, J, dtype):
        """([J, 3] reference positions, [J] their w) of nodes 1..J, or None without the distance term."""
        if self.distance_weight == 0.0:
            return None
        p = np.asarray(self.positions, dtype=np.float32).reshape(-1, 4)[2 if self.node_slot else 0:][:J]
        return p[:, :3].astype(dtype), p[:, 3].astype(dtype)

    def penalised(self):
        return self.limit_weight != 0.0 and self.soft_lo is not None and self.soft_hi is not None


def _setup(chain, x, mask, dtype):
    full = tp.expand(chain, np.asarray(x, dtype=np.float32), mask)
    n, J = len(full), len(chain) - 1
    p, R = frames64.node_frames(chain, full, dtype)
    o = np.asarray(chain["rotation"][0], dtype=dtype)
    R0 = frames64._rot(0, o[0:1], dtype) @ frames64._rot(1, o[1:2], dtype) @ frames64._rot(2, o[2:3], dtype)
    Rn = [np.broadcast_to(R0, (n, 3, 3))] + [R[:, k] for k in range(J)]                       # by node index
    pn = [np.broadcast_to(np.asarray(chain["position"][0], dtype=dtype), (n, 3))] + [p[:, k] for k in range(J)]
    return full, n, J, pn, Rn


def fitness64(chain, x, rest, targets, terms=Terms(), target_rot=None, rot_weights=None, mask=None,
              dtype=np.float64) -> np.ndarray:
    """[n]: sum_e w_e |p_e - t_e|^2 + (distance_weight / J) sum_k (|p_k - ref_k|^2 + (1 - ref_w_k)^2)
    + (angle_weight / J) sum_d (rest_d - x_d)^2 + limit_weight sum_d max(x_d - soft_hi_d, soft_lo_d - x_d, 0)^2
    + sum_e w_e rot_weights[e] |R_e - target_rot[e]|_F^2.  x, rest [n, D]; targets [n, E, 3]; target_rot
    [n, E, 3, 3]."""
    _, n, J, pn, Rn = _setup(chain, x, mask, dtype)
    eff = tp.effectors(chain)
    w = np.asarray(chain["effector_weight"][eff], dtype=dtype)
    t = np.asarray(targets, dtype=dtype).reshape(n, len(eff), 3)
    xd, rd = np.asarray(x, dtype=dtype), np.asarray(rest, dtype=dtype)
    f = np.zeros(n, dtype=dtype)
    for e, m in enumerate(eff):
        f = f + w[e] * np.sum((pn[m] - t[:, e]) ** 2, axis=1, dtype=dtype)
    refs = terms.refs(J, dtype)
    if refs is not None:
        dist = np.zeros(n, dtype=dtype)
        for k in range(1, J + 1):
            dist = dist + np.sum((pn[k] - refs[0][k - 1]) ** 2, axis=1, dtype=dtype) + (dtype(1.0) - refs[1][k - 1]) ** 2
        f = f + dtype(dtype(terms.distance_weight) / dtype(J)) * dist
    f = f + dtype(dtype(terms.angle_weight) / dtype(J)) * np.sum((rd - xd) ** 2, axis=1, dtype=dtype)
    if terms.penalised():
        lo, hi = np.asarray(terms.soft_lo, dtype=dtype), np.asarray(terms.soft_hi, dtype=dtype)
        over = np.maximum(np.maximum(xd - hi, lo - xd), dtype(0.0))
        f = f + dtype(terms.limit_weight) * np.sum(over ** 2, axis=1, dtype=dtype)
    if target_rot is not None and rot_weights is not None:
        rw = np.asarray(rot_weights, dtype=dtype).reshape(len(eff))
        T = np.asarray(target_rot, dtype=dtype).reshape(n, len(eff), 3, 3)
        for e, m in enumerate(eff):
            if rw[e] != 0:  # a weight of 0 never reads its target
                f = f + (w[e] * rw[e]) * np.sum((Rn[m] - T[:, e]) ** 2, axis=(1, 2), dtype=dtype)
    return f


def _vee2(M):
    """v(M) = (M32 - M23, M13 - M31, M21 - M12) of [n, 3, 3]."""
    return np.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], axis=-1)


def gradient64(chain, x, rest, targets, terms=Terms(), target_rot=None, rot_weights=None, mask=None,
               dtype=np.float64, parts=False):
    """[n, D]: d fitness64 / d x, by the header's closed form, one (free dimension, node below it) pair at a
    time.  parts=True returns the dict of the five terms' gradients instead of their sum."""
    full, n, J, pn, Rn = _setup(chain, x, mask, dtype)
    ang = np.asarray(full, dtype=dtype).reshape(n, J, 3)
    free, eff = tp.free_axes(chain, mask), tp.effectors(chain)
    slot = {int(m): e for e, m in enumerate(eff)}
    w = np.asarray(chain["effector_weight"], dtype=dtype)
    t = np.asarray(targets, dtype=dtype).reshape(n, len(eff), 3)
    xd, rd = np.asarray(x, dtype=dtype), np.asarray(rest, dtype=dtype)
    refs = terms.refs(J, dtype)
    rw = None if target_rot is None or rot_weights is None else np.asarray(rot_weights, dtype=dtype).reshape(len(eff))
    T = None if rw is None else np.asarray(target_rot, dtype=dtype).reshape(n, len(eff), 3, 3)
    below = {k: [m for m in range(1, J + 1) if k in jacobian64.ancestors(chain, m)] for k in range(1, J + 1)}
    out = {name: np.zeros((n, len(free)), dtype=dtype) for name in ("position", "distance", "angle", "penalty", "rotation")}
    two = dtype(2.0)
    for d, (k, c) in enumerate(free):
        par = int(chain["parent_index"][k])
        if c == 0:
            a = Rn[par][:, :, 0]
        elif c == 1:
            a = (Rn[par] @ frames64._rot(0, ang[:, k - 1, 0], dtype))[:, :, 1]
        else:
            a = Rn[k][:, :, 2]
        for m in below[k]:
            lever = np.cross(a, pn[m] - pn[par]).astype(dtype)
            if m in slot:
                e = slot[m]
                out["position"][:, d] += two * w[m] * np.sum((pn[m] - t[:, e]) * lever, axis=1, dtype=dtype)
                if rw is not None and rw[e] != 0:
                    v = _vee2(Rn[m] @ np.swapaxes(T[:, e], -1, -2))
                    out["rotation"][:, d] += two * (w[m] * rw[e]) * np.sum(a * v, axis=1, dtype=dtype)
            if refs is not None:
                dw = dtype(dtype(terms.distance_weight) / dtype(J))
                out["distance"][:, d] += two * dw * np.sum((pn[m] - refs[0][m - 1]) * lever, axis=1, dtype=dtype)
        out["angle"][:, d] = two * dtype(dtype(terms.angle_weight) / dtype(J)) * (xd[:, d] - rd[:, d])
        if terms.penalised():
            lo, hi = dtype(terms.soft_lo[d]), dtype(terms.soft_hi[d])
            up, dn = xd[:, d] - hi, lo - xd[:, d]
            lw2 = two * dtype(terms.limit_weight)
            out["penalty"][:, d] = np.where(np.maximum(up, dn) > 0, np.where(up >= dn, lw2 * up, -(lw2 * dn)), dtype(0.0))
    if parts:
        return out
    return (((out["position"] + out["distance"]) + out["rotation"]) + out["angle"]) + out["penalty"]


def subtree_has_effector(chain, mask=None) -> np.ndarray:
    """[D] bool: does free dimension d's node have an effector of non-zero weight in its subtree?"""
    eff = [int(m) for m in tp.effectors(chain) if float(chain["effector_weight"][m]) != 0.0]
    return np.array([any(k in jacobian64.ancestors(chain, m) for m in eff) for k, _ in tp.free_axes(chain, mask)])
