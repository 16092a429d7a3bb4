"""Every compiled kernel width on the GPU, held to the oracle (chains: tests/topologies.py).

visit_topology (csrc/ikpso_swarm.h) routes a parsed chain to one of about 150 instantiations:
TopoGeneric<1..20> and TopoSerialTip<6..14, 20> in both arithmetics, TopoDH<3..12> in FAST, each
with resident, stopping, track, streaming and evaluate builds (and the cooperative kernels of the
serial chains).  The code changes across the widths -- 1024 lanes up to J = 10 and 256 above, the
free-axis mask's bit 59 at J = 20, run-time parents in the generic builds -- and the rest of the
suite touches four of them.  This module runs every width through at least the resident REFERENCE
solve, bit for bit against the oracle on identical seeds, and the edge widths through the other
families; every case asserts the family and topology `s.kernel` names, so a routing change
cannot move a case onto another build unnoticed.  Cases are small: 3 swarms and 6 iterations (4 and
5 in the FAST solves, so that 3 of 4 can be gated in); the track cases take tests/test_gpu_track.py's
path_targets as they are, 24 swarms of 65 particles.

Tolerances, none taken from the code under test:
  * REFERENCE: angles, fitness and generator states bit for bit; residual 1e-5 (as the parity tests).
  * FAST evaluate: node k within 2e-5 max(1, depth(k) / 7) of the float64 FK (2e-5 is the project's
    FAST bound on the 7-deep reference scene; each composed rotation adds one bounded perturbation
    times a lever arm no longer than the capped reach, so the bound grows linearly in depth);
    fitness within relative 1e-5 max(1, depth_max / 7) of the oracle's.
  * FAST solves: generator states bit for bit; the oracle's fitness of the reported angles within
    relative 1e-4 of the reported fitness (test_config5_chain_with_penalty's figure); answers finite
    and inside the clamp bounds; |dtheta| <= 1e-4 on the swarms the tier-A gate lets in (the oracle
    and its FMA-contracted build within 1e-6 rad; at least 3 of 4, tests/test_topologies.py).
  * Folded chain: |dtheta| <= 1e-4 and |df|/f <= 1e-5 at I = 5, tool within 2e-5 of the textbook
    DH product (tests/test_gpu_mask.py's figures).
Measured maxima per width: DESIGN.md §3.
"""
import numpy as np
import pytest

import ikpso
from ikpso import _abi
from ikpso.dh import dh_forward

import topologies as tp
from test_gpu_track import REACHABLE, check_track, median_threshold, path_targets

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, I, P65 = tp.B, tp.ITER, tp.P_SMALL
_CACHE = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def words(states):
    return states.view(np.int32).reshape(-1, 12)[:, :6]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def chain_of(name):
    if name not in _CACHE:
        _CACHE[name] = tp.sweep_chain(name)
    return _CACHE[name]


def dh_case(N):
    if ("dh", N) not in _CACHE:
        arm, a, alpha, d = tp.dh_arm_n(N)
        _CACHE["dh", N] = (arm, arm.origin.to_cuda(), arm.axis_mask, a, alpha, d)
    return _CACHE["dh", N]


def pso(iterations):
    return ikpso.PSOConfig(0.5, 0.5, 1.25, iterations)


def gpu_solve(case, chain, tg, P, iterations, arith, kernel, mask=None, start=None, **kw):
    """(angles, fitness, residual, generator state words, kernel name after the solve)."""
    s = ikpso.BatchSolver(chain, P, pso=pso(iterations), arith=arith, kernel=kernel, axis_mask=mask, **kw)
    nb = tg.shape[0]
    s.seed(nb)
    out = [t.cpu().numpy() for t in s.solve(dev(tg), iterations=iterations,
                                            start_pose=None if start is None else dev(start))]
    out.append(s.generator_states(0, nb)[:, :6])
    name = s.kernel
    s.close()
    print(f"[kernel] {case} {arith} P={P} B={nb}: {name}")
    return out, name


def check_reference(oracle, case, chain, tg, P, kernel, family, topo, mask=None, start=None, iterations=I, **kw):
    """One REFERENCE solve against oracle.solve_batch on identical seeds, bit for bit."""
    (ang, fit, res, states), name = gpu_solve(case, chain, tg, P, iterations, "reference", kernel, mask, start, **kw)
    assert topo in name and family in name, name
    nb, D = tg.shape[0], len(tp.free_axes(chain, mask))
    ostate = oracle.init_generators(nb * P, 0)
    oang, ofit, ores = oracle.solve_batch(chain, tg, start, P, iterations, ostate, threads=4, axis_mask=mask, **kw)
    assert ang.shape == (nb, D)
    assert np.array_equal(bits(ang), bits(oang)), np.argwhere(bits(ang) != bits(oang))[:8].tolist()
    assert np.array_equal(bits(fit), bits(ofit))
    assert np.array_equal(states, words(ostate))
    assert np.array_equal(states, words(oracle.skipahead(oracle.init_generators(nb * P, 0), D + 3 * D * iterations)))
    assert np.max(np.abs(res - ores)) < 1e-5
    return name


def serial_j(name):
    return int(name[len("serial"):])


SERIAL_EDGE = [f"serial{J}" for J in tp.SERIAL_EDGE]


# ------------------------------------------------------------- REFERENCE, bit for bit
@pytest.mark.parametrize("name", tp.sweep_names())
def test_reference_resident(oracle, device, name):
    """P = 65 (a second wave with one lane) on the resident kernel: every generic J = 1..20, every
    serial build, and the serial chains of 5 and 15 joints that fall through to the generic ones."""
    chain = chain_of(name)
    check_reference(oracle, name, chain, tp.solve_targets(chain, B), P65, "resident", "swarm_resident",
                    tp.euler_topology(chain))


@pytest.mark.parametrize("name", tp.edge_names())
def test_reference_full_workgroup_and_one_above(oracle, device, name):
    """The full workgroup (1024 lanes up to J = 10, 256 above), and one particle more, where AUTO
    must leave the resident family: cooperative for the serial chains, streaming for the trees."""
    chain = chain_of(name)
    tg, full = tp.solve_targets(chain, B), tp.full_workgroup(3 * (len(chain) - 1))
    topo = tp.euler_topology(chain)
    check_reference(oracle, name, chain, tg, full, "resident", "swarm_resident", topo)
    with pytest.raises(_abi.IkpsoError) as e:
        ikpso.BatchSolver(chain, full + 1, arith="reference", kernel="resident")
    assert e.value.status == _abi.IKPSO_ERR_UNSUPPORTED
    got = check_reference(oracle, name, chain, tg, full + 1, "auto",
                          "swarm_coop" if name.startswith("serial") else "swarm_streaming", topo)
    assert "resident" not in got


@pytest.mark.parametrize("name", tp.edge_names())
def test_reference_streaming(oracle, device, name):
    chain = chain_of(name)
    check_reference(oracle, name, chain, tp.solve_targets(chain, B), 300, "streaming", "swarm_streaming",
                    tp.euler_topology(chain))


@pytest.mark.parametrize("name", SERIAL_EDGE)
def test_reference_cooperative_two_chunks(oracle, device, name):
    """kernel="coop" with a swarm of two chunks (1024-lane chunks up to J = 10, 256-lane above)."""
    chain = chain_of(name)
    P = 1100 if serial_j(name) <= 10 else 300
    got = check_reference(oracle, name, chain, tp.solve_targets(chain, B), P, "coop", "swarm_coop",
                          tp.euler_topology(chain))
    assert got == f"swarm_coop{tp.euler_topology(chain)}", got  # the throughput plan


@pytest.mark.parametrize("name", SERIAL_EDGE + ["serial7"])
def test_reference_auto_one_swarm(oracle, device, name):
    """kernel="auto" with one swarm: the 1024-lane builds (J <= 10) take the cooperative latency
    variant, with the generators on waves of their own while D <= 21 (J = 6, 7).  The 256-lane
    builds (J >= 11) have no separate latency build: AUTO runs a swarm of one chunk on the
    cooperative kernel itself, whatever the number of swarms, and the name must say so (it said
    swarm_resident until this sweep: DESIGN.md §3)."""
    chain, J = chain_of(name), serial_j(name)
    topo = tp.euler_topology(chain)
    got = check_reference(oracle, name, chain, tp.solve_targets(chain, 1), P65, "auto", "swarm_coop", topo)
    if J <= 10:
        assert got == "swarm_coop" + topo + (" (latency variant, generator waves)" if J <= 7 else " (latency variant)")
    else:
        assert got == "swarm_coop" + topo, got
        got = check_reference(oracle, name, chain, tp.solve_targets(chain, B), P65, "auto", "swarm_coop", topo)
        assert got == "swarm_coop" + topo, got
        # the stopping and track calls of the same solver run (and name) the resident kernel
        s = ikpso.BatchSolver(chain, P65, pso=pso(I), arith="reference", kernel="auto")
        s.seed(B)
        s.solve(dev(tp.solve_targets(chain, B)), iterations=I)
        assert s.kernel == "swarm_coop" + topo, s.kernel
        s.solve_until(dev(tp.solve_targets(chain, B)), max_iterations=I, stop_fitness=-1.0)
        assert s.kernel == "swarm_resident" + topo, s.kernel
        s.close()


@pytest.mark.parametrize("J", tp.GENERIC_EDGE)
def test_reference_masked_generic(oracle, device, J):
    """A random axis mask with a fully locked node (J > 1), a per-swarm start pose and the soft-limit
    penalty over the free angles; at J = 20 node 20's z angle is free: bit 59 of the free mask."""
    chain = chain_of(f"generic{J}")
    rng = np.random.default_rng([J, 11])
    mask = np.concatenate([[0], rng.integers(1, 8, J)]).astype(np.uint8)
    if J > 1:
        mask[3] = 0
    else:
        mask[1] = 5  # its x and z angles
    if J == 20:
        mask[20] |= 4
        assert tp.free_axes(chain, mask)[-1] == (20, 2)
    free = tp.free_axes(chain, mask)
    assert 0 < len(free) < 3 * J  # something to optimise, something locked: the masked build
    lo = np.array([chain["min_rotation"][k][c] for k, c in free], np.float32)
    hi = np.array([chain["max_rotation"][k][c] for k, c in free], np.float32)
    start = tp.random_poses(chain, B, rng, mask)
    got = check_reference(oracle, f"generic{J} masked", chain, tp.solve_targets(chain, B), P65, "resident",
                          "swarm_resident", "<generic>", mask=mask, start=start, limit_weight=10.0,
                          soft_lo=lo + 0.25 * (hi - lo), soft_hi=hi - 0.25 * (hi - lo))
    assert "generic" in got


# --------------------------------------------------------- evaluate, both arithmetics
@pytest.mark.parametrize("name", tp.sweep_names())
def test_evaluate(oracle, device, report, name):
    chain = chain_of(name)
    J, n = len(chain) - 1, 256
    rng = np.random.default_rng([J, 21])
    ang = tp.random_poses(chain, n, rng)
    tg = rng.uniform(-3.0, 3.0, (n, len(tp.effectors(chain)), 3)).astype(np.float32)
    ofit = np.array([oracle.fitness(tp.with_targets(chain, tg[i]), ang[i]) for i in range(n)], np.float32)
    opos = np.array([oracle.node_positions(chain, a) for a in ang], np.float32)
    out = {}
    for arith in ("reference", "fast"):
        s = ikpso.BatchSolver(chain, 64, arith=arith)
        assert tp.euler_topology(chain) in s.kernel, s.kernel
        out[arith] = [t.cpu().numpy() for t in s.evaluate(dev(ang), dev(tg))]
        print(f"[kernel] {name} evaluate {arith}: {s.kernel}")
        s.close()
    fit, pos = out["reference"]
    assert np.array_equal(bits(fit), bits(ofit)) and np.array_equal(bits(pos), bits(opos))
    fit, pos = out["fast"]
    dep = tp.depth(chain)
    err = np.max(np.abs(pos.astype(np.float64) - tp.fk64(chain, ang)), axis=(0, 2))  # per node
    bound = 2e-5 * np.maximum(1.0, dep / 7.0)
    rel = np.abs(fit.astype(np.float64) - ofit) / ofit
    rel_bound = 1e-5 * max(1.0, dep.max() / 7.0)
    report("topologies_evaluate_" + name, {"J": J, "depth_max": int(dep.max()), "fast_pos_max": float(err.max()),
                                           "fast_pos_bound_at_max": float(bound[np.argmax(err)]),
                                           "fast_fit_rel_max": float(rel.max()), "fast_fit_rel_bound": rel_bound})
    assert np.isfinite(pos).all() and (err <= bound).all(), (err / bound).max()
    assert rel.max() <= rel_bound


# ------------------------------------------------------------------------ FAST solves
@pytest.mark.parametrize("name", tp.sweep_names())
def test_fast_solves(oracle, device, name):
    chain = chain_of(name)
    tg = tp.solve_targets(chain, tp.FAST_B)
    lo, hi = chain["min_rotation"][1:].reshape(-1), chain["max_rotation"][1:].reshape(-1)
    for P in tp.fast_sizes(name, chain):
        gated, oang, ofit, _, ostate = tp.tier_a_gate(oracle, chain, tg, P, tp.FAST_I)
        assert gated.mean() >= tp.GATE_SHARE  # the gate leaves out no more than the CPU test allows
        (ang, fit, res, states), got = gpu_solve(name, chain, tg, P, tp.FAST_I, "fast", "resident")
        assert "swarm_resident" in got and tp.euler_topology(chain) in got, got
        assert np.array_equal(states, words(ostate))
        assert np.isfinite(ang).all() and np.isfinite(fit).all() and np.isfinite(res).all()
        assert (ang >= lo).all() and (ang <= hi).all()
        own = np.array([oracle.fitness(tp.with_targets(chain, tg[b]), ang[b]) for b in range(len(tg))], np.float64)
        assert np.max(np.abs(own - fit) / own) <= 1e-4
        dth = np.max(np.abs(ang - oang), axis=1)
        print(f"fast solve {name} P={P}: gated {int(gated.sum())}/{len(gated)}, |dtheta| max {dth[gated].max():.2e}")
        assert (dth[gated] <= 1e-4).all(), dth


# ----------------------------------------------------------------------- folded chain
@pytest.mark.parametrize("N", tp.DH_COMPILED)
def test_folded_chain(oracle, device, report, N):
    arm, chain, mask, a, alpha, d = dh_case(N)
    rng = np.random.default_rng([N, 31])
    # evaluate: the tool against the textbook product
    x = tp.random_poses(chain, 256, rng, mask)
    s = ikpso.BatchSolver(chain, P65, pso=pso(tp.FAST_I), axis_mask=mask, kernel="resident")
    assert f"swarm_resident<dh{N}>" == s.kernel and s.dof == N, s.kernel
    pos = s.evaluate(dev(x))[1].cpu().numpy()
    s.close()
    tool = np.array([dh_forward(arm.joint_angles(v), d, a, alpha) for v in x])
    err = float(np.max(np.abs(pos[:, -1] - tool)))
    report(f"topologies_dh{N}", {"nodes": len(chain) - 1, "tool_max": err, "bound": 2e-5})
    assert err <= 2e-5
    # tier A at I = 5 on the gated swarms
    tg = tp.solve_targets(chain, tp.FAST_B, mask)
    gated, oang, ofit, _, ostate = tp.tier_a_gate(oracle, chain, tg, P65, tp.FAST_I, mask)
    assert gated.mean() >= tp.GATE_SHARE
    (ang, fit, res, states), got = gpu_solve(f"dh{N}", chain, tg, P65, tp.FAST_I, "fast", "resident", mask)
    assert got == f"swarm_resident<dh{N}>", got
    assert np.array_equal(states, words(ostate))
    assert np.isfinite(ang).all() and (np.abs(ang[gated] - oang[gated]) <= 1e-4).all()
    assert (np.abs(fit[gated] - ofit[gated]) / ofit[gated] <= 1e-5).all()
    # the REFERENCE solve of the same masked chain: the Euler kernels, bit for bit
    check_reference(oracle, f"dh{N} unfolded", chain, tg[:B], P65, "resident", "swarm_resident",
                    tp.euler_topology(chain), mask=mask)


@pytest.mark.parametrize("N", (2, 13))
def test_no_folded_build_keeps_the_euler_kernels(oracle, device, N):
    """2 or 13 free angles have no TopoDH build: the FAST solver stays on the masked Euler chain."""
    arm, chain, mask, a, alpha, d = dh_case(N)
    tg = tp.solve_targets(chain, B, mask)
    (ang, fit, res, states), got = gpu_solve(f"dh{N}", chain, tg, P65, tp.FAST_I, "fast", "resident", mask)
    assert got == "swarm_resident" + tp.euler_topology(chain) and "dh" not in got, got
    assert ang.shape == (B, N) and np.isfinite(ang).all() and np.isfinite(fit).all()
    assert np.array_equal(states, words(oracle.skipahead(oracle.init_generators(B * P65, 0), N + 3 * N * tp.FAST_I)))
    own = np.array([oracle.fitness_mask(tp.with_targets(chain, tg[b]), ang[b], mask) for b in range(B)], np.float64)
    assert np.max(np.abs(own - fit) / own) <= 1e-4


# -------------------------------------------------------- track and stopping builds
TRACK_T, TRACK_I = 4, 8
TRACK_CASES = [(f"generic{J}", ar) for J in tp.GENERIC_EDGE for ar in ("reference", "fast")] + \
              [(f"serial{J}", ar) for J in (6, 14) for ar in ("reference", "fast")] + \
              [(f"dh{N}", "fast") for N in tp.DH_EDGE]


@pytest.mark.parametrize("name,arith", TRACK_CASES)
def test_track_equals_the_loop_of_solve_until(device, name, arith):
    """solve_track against the loop of solve_until calls, bit for bit (check_track): for these
    widths the only test of either build, and of solve_until's iteration counts.  The threshold is
    the median fitness of the reachable cells of the non-stopping checker loop."""
    if name.startswith("dh"):
        _, chain, mask = dh_case(int(name[2:]))[:3]
        topo = f"<{name}>"
    else:
        chain, mask = chain_of(name), None
        topo = tp.euler_topology(chain)

    def make():
        return ikpso.BatchSolver(chain, P65, pso=pso(TRACK_I), arith=arith, kernel="resident", axis_mask=mask)

    key = ("track", name)
    if key not in _CACHE:
        _CACHE[key] = path_targets(chain, mask, frames=TRACK_T)
    targets = _CACHE[key]
    stop = median_threshold(make, targets, iterations=TRACK_I)
    got, _, kname = check_track(make, targets, stop, iterations=TRACK_I)
    print(f"[kernel] {name} track {arith}: {kname}")
    assert "swarm_resident" in kname and topo in kname, kname
    n = got[3]
    assert (n < TRACK_I).any(), n.tolist()
    assert (got[1][n < TRACK_I] <= stop).all()
    assert (n[:, REACHABLE:] == TRACK_I).all()  # targets at ten times the reach never stop


# ----------------------------------------------------------------------------- limits
@pytest.mark.parametrize("J,status", [(21, _abi.IKPSO_ERR_UNSUPPORTED), (32, _abi.IKPSO_ERR_UNSUPPORTED),
                                      (33, _abi.IKPSO_ERR_INVALID_ARG)])
def test_chains_beyond_the_compiled_widths(device, J, status):
    """More than 20 joints have no kernel, more than 32 no node table: refused when the solver is
    created (parse time), in both arithmetics, whatever the tree."""
    for chain in (tp.serial(J), tp.random_tree(J, 0)):
        for arith in ("reference", "fast"):
            with pytest.raises(_abi.IkpsoError) as e:
                ikpso.BatchSolver(chain, P65, arith=arith)
            assert e.value.status == status, (J, arith, e.value.status)
