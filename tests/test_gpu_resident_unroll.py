"""The reference scene's resident FAST kernel against bytes recorded before its iteration loop
was unrolled (tests/golden/resident_unroll.npz, written by tests/golden/gen_resident_unroll.py at
commit 4c25385).

The unrolled loop renames registers and removes copies; rounding and operation order are the
rolled loop's, so every comparison here is on bit patterns.  Iterations 0, 1, 2, 3, 5, 6, 11: no
iteration, the remainder alone, one unrolled pair, pair + remainder, and both residues of longer
unrolls; particles 64, 65, 1024: one full wave, a second wave with one active lane, the headline's
16 waves.  The generator states are compared through their SHA-256 (the fixture holds the digest of
the int32 array BatchSolver.generator_states returns).

The residual is part of the comparison for a reason: it is computed after the loop by FAST source
whose sums of products the compiler contracts as it sees fit, and a first form of the unrolled loop
(the iteration as a lambda over the kernel's locals) made it fuse the other product of such sums --
the residual of one swarm came out 1-2 ulp away in (P, I) = (64, 3), (65, 3) and (1024, 5), in the
plain kernel and the stopping twin alike, with angles, fitness and states unchanged.
"""
import hashlib

import numpy as np
import pytest

import ikpso

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 4
ITERATIONS = (0, 1, 2, 3, 5, 6, 11)
PARTICLES = (64, 65, 1024)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def digest(states):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(states).tobytes()).digest(), dtype=np.uint8)


@pytest.fixture(scope="module")
def fixture(golden):
    with np.load(golden / "resident_unroll.npz", allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def wl():
    return ikpso.workload(3)


@pytest.fixture(scope="module")
def targets(device, wl):
    return torch.from_numpy(np.ascontiguousarray(wl.targets(0, B))).cuda()


@pytest.fixture(scope="module", params=PARTICLES)
def solver(request, device, wl):
    s = ikpso.BatchSolver(wl.chain, request.param, pso=wl.pso, fit=wl.fit, kernel="resident")
    yield s
    s.close()


def check(fixture, tag, s, out):
    ang, fit, res = (t.cpu().numpy() for t in out[:3])
    states = digest(s.generator_states(0, B))
    assert np.array_equal(bits(ang), bits(fixture["ang_" + tag])), tag
    assert np.array_equal(bits(fit), bits(fixture["fit_" + tag])), tag
    assert np.array_equal(bits(res), bits(fixture["res_" + tag])), tag
    assert np.array_equal(states, fixture["rng_" + tag]), tag


@pytest.mark.parametrize("I", ITERATIONS)
def test_plain_matches_fixture(fixture, solver, targets, I):
    solver.seed(B, seed_base=0)
    out = solver.solve(targets, iterations=I)
    assert "resident" in solver.kernel and "ref_tree7" in solver.kernel, solver.kernel
    check(fixture, f"P{solver.P}_I{I}", solver, out)


@pytest.mark.parametrize("I", ITERATIONS)
def test_until_matches_fixture(fixture, solver, targets, I):
    """The stopping twin with a threshold of 0 (never met) and an iteration output: every swarm runs
    I iterations and returns the plain kernel's bytes."""
    solver.seed(B, seed_base=0)
    out = solver.solve_until(targets, max_iterations=I, stop_fitness=0.0)
    assert "resident" in solver.kernel, solver.kernel
    assert (out[3].cpu().numpy() == I).all()
    check(fixture, f"P{solver.P}_I{I}", solver, out)


def test_second_call_matches_fixture(fixture, device, wl, targets):
    """Two consecutive solves on one solver: the second starts from the states the first one's
    remainder iteration stored."""
    P, I = 1024, 3
    with ikpso.BatchSolver(wl.chain, P, pso=wl.pso, fit=wl.fit, kernel="resident") as s:
        s.seed(B, seed_base=0)
        check(fixture, f"P{P}_I{I}", s, s.solve(targets, iterations=I))
        check(fixture, f"P{P}_I{I}_second", s, s.solve(targets, iterations=I))
