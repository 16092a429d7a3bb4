"""The aim fitness in numpy float64, from the node table and the definitions alone (include/ikpso.h:
ikpso_solve_track_aim) on top of tests/pose64.py.  Test infrastructure, imported like
tests/pose64.py; nothing here touches a GPU or the library."""
import numpy as np

import pose64


def unit(axis) -> np.ndarray:
    a = np.asarray(axis, dtype=np.float64)
    return a / np.linalg.norm(a)


def aim_fitness(chain, mask, angle_weight, answers, rest, targets, axis, dirs, weight) -> np.ndarray:
    """[n] float64 fitness of free-axis answers [n, D] as the header states it: the position and angle
    terms as pose64.pose_fitness states them (the tip term w_e |p - t|^2 and (angle_weight / J)
    sum (rest - x)^2), plus w_e * weight * |R_eff a - d|^2 with a = axis / |axis| in the effector
    node's frame and d = dirs [n, 3] as given."""
    J = len(chain) - 1
    w_e = float(chain["effector_weight"][J])
    p, R = pose64.poses(chain, answers, mask)
    t = np.asarray(targets, dtype=np.float64).reshape(len(p), 3)
    d = np.asarray(dirs, dtype=np.float64).reshape(len(p), 3)
    x, r = np.asarray(answers, dtype=np.float64), np.asarray(rest, dtype=np.float64)
    position = w_e * np.sum((p - t) ** 2, axis=1)
    angle = (float(angle_weight) / J) * np.sum((r - x) ** 2, axis=1)
    aim = w_e * float(weight) * np.sum((R @ unit(axis) - d) ** 2, axis=1)
    return position + angle + aim


def aim_angle(R, axis, dirs) -> np.ndarray:
    """[n] angle between R a and the unit directions dirs [n, 3], from the chord
    |R a - d| = 2 sin(phi / 2) (well conditioned at small angles, where the dot product is not)."""
    chord = np.linalg.norm(np.asarray(R, np.float64) @ unit(axis) - np.asarray(dirs, np.float64), axis=-1)
    return 2.0 * np.arcsin(np.clip(chord / 2.0, 0.0, 1.0))
