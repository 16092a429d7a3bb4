"""Chains for the sweep over every compiled kernel width (tests/test_topologies.py on the CPU,
tests/test_gpu_topologies.py on the GPU), and the independent float64 forward kinematics both are
held to.  Test infrastructure, imported like tests/tierb.py; nothing here touches a GPU.

  * random_tree(J, seed): a random tree of J joints with several effectors -> TopoGeneric<J>;
  * serial(J): ikpso.serial_chain(J, length) -> TopoSerialTip<J> where compiled, else TopoGeneric<J>;
  * dh_arm_n(N, seed): an N-joint standard-DH arm; with its axis mask a FAST solver folds it to
    TopoDH<N> for N = 3..12;
  * fk64(chain, angles): node positions from the definition in numpy float64.

Every chain's longest root-to-node path is capped at the reference scene's (reach_cap()), so the
tolerances stated for that scene carry over with the depth as their only scale.
"""
import numpy as np

import ikpso
from ikpso._abi import NODE, NODE_DTYPE, NODE_EFFECTOR, NODE_ORIGIN
from ikpso.dh import dh_arm

REF7_PARENTS = [-1, 0, 1, 2, 3, 4, 4, 4]
SERIAL_COMPILED = (6, 7, 8, 9, 10, 11, 12, 13, 14, 20)  # TopoSerialTip<J> instantiations
DH_COMPILED = tuple(range(3, 13))                        # TopoDH<N> instantiations


# ------------------------------------------------------------------ chain geometry
def path_lengths(chain) -> np.ndarray:
    """Per node (origin included, index 0), the sum of |link length| from the root (float64)."""
    out = np.zeros(len(chain))
    for k in range(1, len(chain)):
        out[k] = out[int(chain["parent_index"][k])] + abs(float(chain["length"][k]))
    return out


def reach_cap() -> float:
    """Longest root-to-node path of the reference scene (its five unit links)."""
    return float(path_lengths(ikpso.reference_scene(reset=True).origin.to_cuda()).max())


def depth(chain) -> np.ndarray:
    """Joints on the path from the root to node k, for k = 1..J (row k-1, as fk64's rows)."""
    d = np.zeros(len(chain), dtype=np.int64)
    for k in range(1, len(chain)):
        d[k] = d[int(chain["parent_index"][k])] + 1
    return d[1:]


def effectors(chain) -> np.ndarray:
    """Node indices of the effectors, in node order (the order of a solver's targets)."""
    return np.flatnonzero(chain["node_type"] == NODE_EFFECTOR)


def is_serial_tip(chain) -> bool:
    J = len(chain) - 1
    return chain["parent_index"].tolist() == list(range(-1, J)) and effectors(chain).tolist() == [J]


def is_ref7(chain) -> bool:
    return chain["parent_index"].tolist() == REF7_PARENTS and effectors(chain).tolist() == [5, 6, 7]


def _cap_scale(longest: float) -> float:
    """Factor that brings a longest path under the cap (never lengthens; a hair under, so the
    float32 lengths' sum stays under it too)."""
    cap = reach_cap()
    return 1.0 if longest <= cap else cap / longest * (1.0 - 1e-6)


# ------------------------------------------------------------------------ the chains
def random_tree(J: int, seed: int) -> np.ndarray:
    """Chain table of a random tree: parent_index[k] uniform in [0, k); every leaf an effector and,
    for J >= 3, one interior joint too (weights in [0.5, 2]); per-axis clamp bounds inside
    [-pi, pi] (the transcendental unit's range: no poly_trig build) with the rest rotation inside
    them; an origin with a position and a rotation; link lengths in [0.2, 1], scaled under the
    cap.  Draws that give a tip-effector serial chain, the reference tree, or (J >= 3) no interior
    joint are redrawn; J = 1 is its one node, an effector."""
    rng = np.random.default_rng([int(J), int(seed)])
    while True:
        parent = np.array([-1] + [int(rng.integers(0, k)) for k in range(1, J + 1)])
        kids = np.bincount(parent[1:], minlength=J + 1)
        leaves = [k for k in range(1, J + 1) if kids[k] == 0]
        interior = [k for k in range(1, J + 1) if kids[k] > 0]
        if J >= 3 and not interior:
            continue
        eff = sorted(leaves + ([int(rng.choice(interior))] if J >= 3 else []))
        if J >= 2 and parent.tolist() == list(range(-1, J)) and eff == [J]:
            continue
        if parent.tolist() == REF7_PARENTS and eff == [5, 6, 7]:
            continue
        break
    c = np.zeros(J + 1, dtype=NODE_DTYPE)
    c["parent_index"] = parent
    c["node_type"] = NODE
    c["node_type"][0] = NODE_ORIGIN
    c["node_type"][eff] = NODE_EFFECTOR
    c["effector_weight"][eff] = rng.uniform(0.5, 2.0, len(eff))
    c["target_position"][eff] = rng.uniform(-2.0, 2.0, (len(eff), 3))
    centre, half = rng.uniform(-2.0, 2.0, (J + 1, 3)), rng.uniform(0.3, 1.0, (J + 1, 3))
    c["min_rotation"], c["max_rotation"] = centre - half, centre + half  # within [-3, 3]
    lo, hi = c["min_rotation"].astype(np.float64), c["max_rotation"].astype(np.float64)
    c["rotation"] = lo + rng.uniform(0.1, 0.9, (J + 1, 3)) * (hi - lo)
    c["position"][0] = rng.uniform(-0.3, 0.3, 3)
    c["length"][1:] = rng.uniform(0.2, 1.0, J)
    c["length"][1:] *= np.float32(_cap_scale(path_lengths(c).max()))
    return c


def serial(J: int) -> np.ndarray:
    """ikpso.serial_chain(J, length) with the link length min(1, cap / J)."""
    return ikpso.serial_chain(J, _cap_scale(float(J)) * 1.0).to_cuda()


def dh_arm_n(N: int, seed: int = 0):
    """(arm, a, alpha, d): an N-joint standard-DH arm (ikpso.dh.dh_arm).  alpha from {+pi/2, -pi/2,
    0}; N // 2 joints have an offset d != 0 (a locked node follows each), about half a link a != 0;
    asymmetric joint limits within +-2.8 rad; the link offsets scaled under the cap.  The node count
    is N + N // 2 (<= 20 up to N = 13)."""
    rng = np.random.default_rng([1000 + int(N), int(seed)])
    alpha = rng.choice([np.pi / 2, -np.pi / 2, 0.0], N)
    d = np.zeros(N)
    d[rng.choice(N, N // 2, replace=False)] = rng.uniform(0.15, 0.5, N // 2) * rng.choice([-1.0, 1.0], N // 2)
    a = rng.uniform(0.15, 0.5, N) * (rng.random(N) < 0.5)
    if not a.any() and not d.any():
        a[-1] = 0.3
    s = _cap_scale(float(np.hypot(a, d).sum()))
    a, d = a * s, d * s
    lo, hi = -rng.uniform(1.0, 2.8, N), rng.uniform(1.0, 2.8, N)
    return dh_arm(a, alpha, d, lo, hi), a, alpha, d


def euler_topology(chain) -> str:
    """The topology name the Euler kernels of a chain carry (ikpso_solver_kernel_name)."""
    J = len(chain) - 1
    if is_ref7(chain):
        return "<ref_tree7>"
    return f"<serial_tip{J}>" if is_serial_tip(chain) and J in SERIAL_COMPILED else "<generic>"


def full_workgroup(dims: int) -> int:
    """Lanes of the resident workgroup of a kernel with `dims` dimensions (3 J, or N folded)."""
    return 1024 if dims <= 30 else 256


# --------------------------------------------------------------- independent reference
def _rot(axis: int, a: np.ndarray) -> np.ndarray:
    """[n, 3, 3] rotations about x, y or z by the angles a [n]."""
    c, s = np.cos(a), np.sin(a)
    m = np.zeros(a.shape + (3, 3))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[..., axis, axis] = 1.0
    m[..., i, i] = c
    m[..., j, j] = c
    m[..., i, j] = -s
    m[..., j, i] = s
    return m


def fk64(chain, full_euler_angles) -> np.ndarray:
    """World positions of nodes 1..J, float64: [J, 3] for one angle vector [3 J], [n, J, 3] for
    [n, 3 J].  From the definition alone: frame(0) = T(origin position) Rx Ry Rz(origin rotation);
    frame(k) = frame(parent(k)) Rx(x_k) Ry(y_k) Rz(z_k) T(length_k, 0, 0); a node's position is its
    frame's translation."""
    ang = np.asarray(full_euler_angles, dtype=np.float64)
    single = ang.ndim == 1
    ang = ang.reshape(1 if single else ang.shape[0], -1, 3)
    n, J = ang.shape[0], len(chain) - 1
    assert ang.shape[1] == J
    o = np.asarray(chain["rotation"][0], dtype=np.float64)
    R = [None] * (J + 1)
    p = [None] * (J + 1)
    R[0] = np.broadcast_to((_rot(0, o[0:1]) @ _rot(1, o[1:2]) @ _rot(2, o[2:3])), (n, 3, 3))
    p[0] = np.broadcast_to(np.asarray(chain["position"][0], dtype=np.float64), (n, 3))
    for k in range(1, J + 1):
        par = int(chain["parent_index"][k])
        R[k] = R[par] @ _rot(0, ang[:, k - 1, 0]) @ _rot(1, ang[:, k - 1, 1]) @ _rot(2, ang[:, k - 1, 2])
        p[k] = p[par] + float(chain["length"][k]) * R[k][:, :, 0]
    out = np.stack(p[1:], axis=1)
    return out[0] if single else out


# ------------------------------------------------------------------ poses and targets
def free_axes(chain, mask=None):
    return [(k, c) for k in range(1, len(chain)) for c in range(3) if mask is None or (int(mask[k]) >> c) & 1]


def random_poses(chain, n: int, rng, mask=None) -> np.ndarray:
    """[n, D] float32 angle vectors over the free axes, each inside its clamp bounds."""
    free = free_axes(chain, mask)
    lo = np.array([chain["min_rotation"][k][c] for k, c in free], dtype=np.float64)
    hi = np.array([chain["max_rotation"][k][c] for k, c in free], dtype=np.float64)
    x = (lo + rng.uniform(0.0, 1.0, (n, lo.size)) * (hi - lo)).astype(np.float32)
    return np.clip(x, lo.astype(np.float32), hi.astype(np.float32))


def expand(chain, angles, mask=None) -> np.ndarray:
    """Full Euler vectors [n, 3 J] of free-axis vectors [n, D] (locked axes at the chain's rotation)."""
    full = np.repeat(np.asarray(chain["rotation"][1:], dtype=np.float32).reshape(1, -1), len(angles), axis=0)
    full[:, [3 * (k - 1) + c for k, c in free_axes(chain, mask)]] = angles
    return full


def reachable_targets(chain, n: int, rng, mask=None) -> np.ndarray:
    """[n, E, 3] float32: the effector positions (fk64) of n random in-bounds poses."""
    pos = fk64(chain, expand(chain, random_poses(chain, n, rng, mask), mask)).reshape(n, -1, 3)
    return np.ascontiguousarray(pos[:, effectors(chain) - 1], dtype=np.float32)


def with_targets(chain, targets) -> np.ndarray:
    """A copy of the chain with one swarm's targets [E, 3] in its effector nodes."""
    c = chain.copy()
    c["target_position"][effectors(chain)] = targets
    return c


# ------------------------------------------------------------------- the sweep's cases
GENERIC_J = tuple(range(1, 21))
SERIAL_J = SERIAL_COMPILED + (5, 15)   # 5 and 15: serial chains without a build of their own -> generic
GENERIC_EDGE, SERIAL_EDGE, DH_EDGE = (1, 10, 11, 20), (6, 10, 11, 14), (3, 12)
B, ITER, P_SMALL = 3, 6, 65            # the REFERENCE sweep's swarms, iterations and small swarm
FAST_B, FAST_I = 4, 5                  # the FAST solves: four swarms, so that "3 of 4 gated in" can hold
TARGET_SEED = 77
GATE_RAD, GATE_SHARE = 1e-6, 0.75


def sweep_names():
    return [f"generic{J}" for J in GENERIC_J] + [f"serial{J}" for J in SERIAL_J]


def edge_names():
    return [f"generic{J}" for J in GENERIC_EDGE] + [f"serial{J}" for J in SERIAL_EDGE]


def sweep_chain(name: str) -> np.ndarray:
    J = int("".join(ch for ch in name if ch.isdigit()))
    return random_tree(J, 0) if name.startswith("generic") else serial(J)


def solve_targets(chain, n: int, mask=None) -> np.ndarray:
    return reachable_targets(chain, n, np.random.default_rng(TARGET_SEED), mask)


def fast_sizes(name: str, chain) -> list:
    """Swarm sizes of the FAST solve test: 65, and the full workgroup at the edge widths."""
    return [P_SMALL] + ([full_workgroup(3 * (len(chain) - 1))] if name in edge_names() else [])


def tier_a_gate(oracle, chain, targets, P: int, I: int, mask=None, **kw):
    """(gated [B] bool, angles, fitness, residual, generator states): the oracle's solve on seeds
    0.., and which swarms its FMA-contracted build answers within GATE_RAD of it -- the swarms on
    which two valid fp32 evaluations still agree, so a third (the GPU's FAST) can be held to 1e-4."""
    nb = targets.shape[0]
    st = oracle.init_generators(nb * P, 0)
    ang, fit, res = oracle.solve_batch(chain, targets, None, P, I, st, threads=4, axis_mask=mask, **kw)
    fang, _, _ = oracle.solve_batch(chain, targets, None, P, I, oracle.init_generators(nb * P, 0), threads=4,
                                    axis_mask=mask, lib=oracle.load_fma(), **kw)
    return np.max(np.abs(ang - fang), axis=1) <= GATE_RAD, ang, fit, res, st
