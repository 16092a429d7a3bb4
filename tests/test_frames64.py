"""tests/frames64.py on the CPU: the float64 restatement the GPU tests of ikpso_solve_track_frames
are held to, itself held to tests/pose64.py on serial chains (tip rotation and position, a second
statement of the same definition) and to the oracle's FK positions on random trees (the parent
handling).  The oracle's bound is tests/test_topologies.py's: correctly rounded fp32 on a reach no
longer than the reference scene's."""
import numpy as np
import pytest

import ikpso

import frames64
import pose64
import topologies as tp

FK_TOL, POSES = 1e-5, 50


@pytest.mark.parametrize("J", (6, 7, 20))
def test_serial_chains_match_pose64(J):
    chain = tp.serial(J)
    x = tp.random_poses(chain, POSES, np.random.default_rng([J, 5]))
    p, R = frames64.effector_frames(chain, x)
    want_p, want_R = pose64.poses(chain, x, None)
    assert p.shape == (POSES, 1, 3) and R.shape == (POSES, 1, 3, 3)
    assert np.max(np.abs(p[:, 0] - want_p)) <= 1e-12 and np.max(np.abs(R[:, 0] - want_R)) <= 1e-12
    assert np.max(np.abs(R[:, 0] @ R[:, 0].transpose(0, 2, 1) - np.eye(3))) <= 1e-12


def test_masked_arm_matches_pose64():
    arm = tp.dh_arm_n(7)[0]
    chain, mask = arm.origin.to_cuda(), arm.axis_mask
    x = tp.random_poses(chain, POSES, np.random.default_rng(6), mask)
    p, R = frames64.effector_frames(chain, x, mask)
    want_p, want_R = pose64.poses(chain, x, mask)
    assert np.max(np.abs(p[:, 0] - want_p)) <= 1e-12 and np.max(np.abs(R[:, 0] - want_R)) <= 1e-12


@pytest.mark.parametrize("J", (1, 3, 7, 20))
def test_random_trees_match_the_oracle(oracle, J):
    worst = 0.0
    for seed in range(2):
        chain = tp.random_tree(J, seed)
        full = tp.random_poses(chain, POSES, np.random.default_rng([J, seed, 7]))
        got, R = frames64.node_frames(chain, full)
        want = np.array([oracle.node_positions(chain, a) for a in full], dtype=np.float64)
        worst = max(worst, float(np.max(np.abs(got - want))))
        assert np.max(np.abs(got - tp.fk64(chain, full))) <= 1e-12
        assert np.max(np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3))) <= 1e-12
    print(f"frames64 vs the oracle, random trees J={J}: max {worst:.2e}")
    assert worst <= FK_TOL


def test_reference_tree_effectors_in_node_order():
    chain = ikpso.reference_scene(reset=True).origin.to_cuda()
    x = tp.random_poses(chain, 4, np.random.default_rng(8))
    p, R = frames64.effector_frames(chain, x)
    allp, allR = frames64.node_frames(chain, x)
    assert tp.effectors(chain).tolist() == [5, 6, 7]
    assert np.array_equal(p, allp[:, 4:7]) and np.array_equal(R, allR[:, 4:7])


def test_fitness_terms():
    """The fitness from its parts: at the answer's own pose only the angle term is left; a weight of
    0 drops its effector's term; the term is w_e rw_e 4 (1 - cos theta) (the chord of the geodesic)."""
    chain = tp.random_tree(7, 0)
    E = len(tp.effectors(chain))
    rng = np.random.default_rng(9)
    x, rest = tp.random_poses(chain, 5, rng), tp.random_poses(chain, 5, rng)
    p, R = frames64.effector_frames(chain, x)
    J = len(chain) - 1
    angle = 3.0 / J * np.sum((rest.astype(np.float64) - x.astype(np.float64)) ** 2, axis=1)
    rw = np.array([1.0, 0.0, 0.5, 2.0][:E] + [1.0] * max(0, E - 4))
    assert np.allclose(frames64.frames_fitness(chain, 3.0, x, rest, p, R, rw), angle, rtol=0, atol=1e-14)
    Rt = R[rng.permutation(5)]
    f = frames64.frames_fitness(chain, 3.0, x, rest, p, Rt, rw)
    w = chain["effector_weight"][tp.effectors(chain)].astype(np.float64)
    want = angle + np.sum(w * rw * 4.0 * (1.0 - np.cos(frames64.geodesic(R, Rt))), axis=1)
    assert np.allclose(f, want, rtol=1e-12, atol=1e-12)
    Rt0 = Rt.copy()
    Rt0[:, rw == 0] = 0.0  # what a weight-0 effector is given does not matter
    assert np.array_equal(frames64.frames_fitness(chain, 3.0, x, rest, p, Rt0, rw), f)
    f32 = frames64.frames_fitness(chain, 3.0, x, rest, p, Rt, rw, dtype=np.float32)
    assert f32.dtype == np.float32 and np.max(np.abs(f32 - f)) <= 1e-4
