"""The CPU side of the sweep over every compiled kernel width (tests/topologies.py):

  * the oracle's FK against an independent float64 FK written from the definition (fk64), on random
    trees of every J = 1..20 and on the serial chains -- until now the oracle's parent handling was
    pinned only on the reference tree (recorded data) and on DH arms (dh_forward);
  * what the generators promise (valid trees, the stated effectors, never serial or the reference
    tree, the reach cap);
  * the tier-A gate of the GPU's FAST solve tests: on which swarms the oracle and its FMA-contracted
    build still agree within 1e-6 rad, and that this is at least 3 of every 4 per chain.

The bound 1e-5 of the FK comparison is not taken from the oracle: it is correctly rounded fp32 on a
reach no longer than the reference scene's, where its error against the reference's recorded
positions has median 1.3e-5.  Measured maxima per J: DESIGN.md §3.
"""
import numpy as np
import pytest

import ikpso
from ikpso.dh import dh_forward

import topologies as tp

FK_TOL, DH_TOL, POSES = 1e-5, 2e-5, 200


def oracle_positions(oracle, chain, full):
    return np.array([oracle.node_positions(chain, a) for a in full], dtype=np.float64)


@pytest.mark.parametrize("J", tp.GENERIC_J)
def test_oracle_fk_random_trees(oracle, J):
    worst = 0.0
    for seed in range(3):
        chain = tp.random_tree(J, seed)
        full = tp.random_poses(chain, POSES, np.random.default_rng([J, seed, 1]))
        worst = max(worst, float(np.max(np.abs(oracle_positions(oracle, chain, full) - tp.fk64(chain, full)))))
    print(f"oracle vs fk64, random trees J={J}: max {worst:.2e}")
    assert worst <= FK_TOL


@pytest.mark.parametrize("J", tp.SERIAL_J)
def test_oracle_fk_serial_chains(oracle, J):
    chain = tp.serial(J)
    full = tp.random_poses(chain, POSES, np.random.default_rng([J, 2]))
    worst = float(np.max(np.abs(oracle_positions(oracle, chain, full) - tp.fk64(chain, full))))
    print(f"oracle vs fk64, serial J={J}: max {worst:.2e}")
    assert worst <= FK_TOL


@pytest.mark.parametrize("N", (2,) + tp.DH_COMPILED + (13,))
def test_oracle_fk_dh_arms(oracle, N):
    """The oracle's (and fk64's) tool position of the marshalled arm against the textbook product."""
    arm, a, alpha, d = tp.dh_arm_n(N)
    chain, mask = arm.origin.to_cuda(), arm.axis_mask
    assert len(chain) - 1 == N + N // 2 and tp.is_serial_tip(chain)
    assert sum(bin(int(m)).count("1") for m in mask) == N
    x = tp.random_poses(chain, POSES, np.random.default_rng([N, 3]), mask)
    full = tp.expand(chain, x, mask)
    want = np.array([dh_forward(arm.joint_angles(v), d, a, alpha) for v in x])
    assert np.max(np.abs(tp.fk64(chain, full)[:, -1] - want)) <= 1e-6  # fp32-rounded node table
    worst = float(np.max(np.abs(oracle_positions(oracle, chain, full)[:, -1] - want)))
    print(f"oracle vs dh_forward, N={N}: max {worst:.2e}")
    assert worst <= DH_TOL


def test_fk64_on_the_reference_scene(fk_kat):
    """fk64 itself against the reference's recorded positions (6 significant digits)."""
    chain = ikpso.reference_scene(reset=True).origin.to_cuda()
    pos = tp.fk64(chain, fk_kat["degrees"]).reshape(len(fk_kat["degrees"]), 21)
    assert np.max(np.abs(pos - fk_kat["positions"])) < 1e-4
    assert tp.is_ref7(chain) and tp.reach_cap() == 5.0 and tp.depth(chain).tolist() == [1, 2, 3, 4, 5, 5, 5]


@pytest.mark.parametrize("J", tp.GENERIC_J)
def test_random_tree_properties(J):
    cap = tp.reach_cap()
    for seed in range(3):
        c = tp.random_tree(J, seed)
        par = c["parent_index"]
        assert len(c) == J + 1 and par[0] == -1 and all(0 <= par[k] < k for k in range(1, J + 1))
        assert c["node_type"][0] == ikpso.NODE_ORIGIN
        kids = np.bincount(par[1:], minlength=J + 1)
        eff = set(tp.effectors(c).tolist())
        leaves = {k for k in range(1, J + 1) if kids[k] == 0}
        assert leaves <= eff and len(eff - leaves) == (1 if J >= 3 else 0)
        assert all(0.5 <= c["effector_weight"][k] <= 2.0 for k in eff)
        assert not tp.is_ref7(c) and (J == 1 or not tp.is_serial_tip(c))
        assert tp.euler_topology(c) == "<generic>"
        lo, hi, rest = c["min_rotation"][1:], c["max_rotation"][1:], c["rotation"][1:]
        assert (lo >= -np.pi).all() and (hi <= np.pi).all() and (lo < rest).all() and (rest < hi).all()
        assert len({(float(a), float(b)) for a, b in zip(lo.ravel(), hi.ravel())}) == 3 * J  # per axis
        assert np.abs(c["position"][0]).max() > 0 and np.abs(c["rotation"][0]).max() > 0
        assert 0.0 < tp.path_lengths(c).max() <= cap
        assert np.array_equal(tp.random_tree(J, seed), c)  # a function of (J, seed)


def test_serial_and_dh_generators():
    cap = tp.reach_cap()
    for J in tp.SERIAL_J:
        c = tp.serial(J)
        assert tp.is_serial_tip(c) and tp.path_lengths(c).max() <= cap
        assert tp.euler_topology(c) == (f"<serial_tip{J}>" if J in tp.SERIAL_COMPILED else "<generic>")
    for N in (2,) + tp.DH_COMPILED + (13,):
        arm, a, alpha, d = tp.dh_arm_n(N)
        c = arm.origin.to_cuda()
        assert len(c) - 1 <= 20 and tp.path_lengths(c).max() <= cap
        assert np.count_nonzero(d) == N // 2 and set(np.round(alpha / (np.pi / 2)).tolist()) <= {-1.0, 0.0, 1.0}


def test_draws_per_solve(oracle):
    """What the GPU tests compare generator states with: a solve draws D + 3 D I uniforms per
    particle over the D free angles, with or without a start pose."""
    chain = tp.random_tree(5, 0)
    mask = np.array([0, 7, 0, 5, 2, 7], np.uint8)
    D, P, I, nb = 9, 33, 4, 2
    tg = tp.solve_targets(chain, nb)
    for start in (None, tp.random_poses(chain, nb, np.random.default_rng(4), mask)):
        st = oracle.init_generators(nb * P, 0)
        oracle.solve_batch(chain, tg, start, P, I, st, axis_mask=mask)
        want = oracle.skipahead(oracle.init_generators(nb * P, 0), D + 3 * D * I)
        assert np.array_equal(st.view(np.int32).reshape(-1, 12)[:, :6], want.view(np.int32).reshape(-1, 12)[:, :6])


def gate_cases():
    for name in tp.sweep_names():
        yield name
    for N in tp.DH_COMPILED:
        yield f"dh{N}"


@pytest.mark.parametrize("name", list(gate_cases()))
def test_tier_a_gate_share(oracle, name):
    """The swarms of the GPU's FAST solve tests, solved by the oracle with and without FMA
    contraction: at least 3 of every 4 agree within 1e-6 rad, for the reference alone."""
    if name.startswith("dh"):
        arm = tp.dh_arm_n(int(name[2:]))[0]
        chain, mask, sizes = arm.origin.to_cuda(), arm.axis_mask, [tp.P_SMALL]
    else:
        chain, mask = tp.sweep_chain(name), None
        sizes = tp.fast_sizes(name, chain)
    tg = tp.solve_targets(chain, tp.FAST_B, mask)
    for P in sizes:
        gated = tp.tier_a_gate(oracle, chain, tg, P, tp.FAST_I, mask)[0]
        print(f"tier-A gate {name} P={P} I={tp.FAST_I}: {int(gated.sum())}/{len(gated)} swarms")
        assert gated.mean() >= tp.GATE_SHARE
