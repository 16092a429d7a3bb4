"""ikpso_solver_evaluate_contacts on the GPU (BatchSolver.contacts): which node hits which collider.

The chains, poses and checkers are tests/contacts_cases.py's (tests/test_contacts.py holds them to their own
conditions on the CPU): 600 poses per chain -- two full 256-lane workgroups and a tail -- uniform in [0, 2 pi).

  1. REFERENCE: every bit equals the oracle's orc_node_collides of that node and that collider alone.
  2. Both arithmetics: some word of a pose is non-zero exactly when evaluate()'s fitness of it is FLT_MAX.
  3. FAST against the float64 separating-axis checker, outside a band around touching.
  4. Pruned colliders keep their columns (zeros); a solver with nothing to test.
  5. out_positions is evaluate()'s.
  6. examples/contacts_c.c builds, runs and reports the pair it pushed together.
"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import contacts_cases as cc
import ikpso
from ikpso import _abi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FMAX = np.float32(np.finfo(np.float32).max)
ARITHS = ("reference", "fast")
EXAMPLES = Path(__file__).resolve().parents[1] / "examples"
# Test 3's band for the chains FAST decides by separating axes: twice the largest |gap| at which a decision
# was seen to differ from the float64 checker's on an MI355X (see test_fast_against_the_float64_checker).
SAT_BAND = 2 * 7.1e-7
# FAST positions: the project's stated bound on FAST frame rounding (tests/test_gpu_collide.py)
FAST_POS_TOL = 2e-5


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def solver(name, arith, boxes=None):
    chain, own, mask = cc.case(name)
    return ikpso.BatchSolver(chain, 64, arith=arith, colliders=own if boxes is None else boxes, axis_mask=mask)


@pytest.fixture(scope="module")
def runs(device):
    """{(case, arith): contacts words, contacts' positions, evaluate's fitness and positions}: one solver per
    case and arithmetic, every test reads from here."""
    out = {}
    for name in cc.NAMES:
        for arith in ARITHS:
            s = solver(name, arith)
            x = dev(cc.poses(name))
            words, pos = s.contacts(x, positions=True)
            fit, epos = s.evaluate(x)
            out[(name, arith)] = dict(words=words.cpu().numpy().view(np.uint32), pos=pos.cpu().numpy(),
                                      fit=fit.cpu().numpy(), epos=epos.cpu().numpy(), kept=s.collider_count)
            s.close()
    return out


def params():
    return [(n, a) for n in cc.NAMES for a in ARITHS]


# --------------------------------------------------------------------------- 1. REFERENCE, bit for bit
@pytest.mark.parametrize("name", cc.NAMES)
def test_reference_bits_are_the_oracles(oracle, runs, name):
    chain, boxes, _ = cc.case(name)
    want, got = cc.oracle_bits(oracle, name), runs[(name, "reference")]["words"]
    assert got.shape == want.shape == (cc.N_POSES, len(boxes))
    share = float((want != 0).any(axis=1).mean())
    print(f"{name}: {int(cc.unpack(want, len(chain) - 1).sum())} contacts, {share:.3f} of the poses collide, "
          f"{int((got != want).sum())} words differ")
    assert 0.05 < share < 0.95  # both outcomes exercised
    if name == "serial20":
        assert ((want >> np.uint32(19)) & 1).any()  # the 20th node's bit
    assert np.array_equal(got, want)


# ----------------------------------------------------------------- 2. consistent with evaluate, exactly
@pytest.mark.parametrize("name,arith", params())
def test_some_contact_exactly_when_evaluate_gives_flt_max(runs, name, arith):
    r = runs[(name, arith)]
    any_contact, hit = (r["words"] != 0).any(axis=1), r["fit"] == FMAX
    print(f"{name} {arith}: {int(hit.sum())} of {cc.N_POSES} poses at FLT_MAX, {int((any_contact != hit).sum())} differ")
    assert 0 < hit.sum() < cc.N_POSES
    assert np.array_equal(any_contact, hit)


def test_a_collider_that_is_no_rotation_takes_gjk_in_fast(device):
    """A quaternion of norm 1.05 is no rotation: the FAST solver tests the whole scene by GJK (the masked
    collider builds), and contacts() follows it there."""
    chain, boxes, _ = cc.case("scene4")
    boxes = boxes.copy()
    boxes[3]["quat"] = boxes[3]["quat"] * np.float32(1.05)
    x = dev(cc.poses("scene4"))
    with ikpso.BatchSolver(chain, 64, arith="fast", colliders=boxes) as s:
        words = s.contacts(x).cpu().numpy()
        fit = s.evaluate(x)[0].cpu().numpy()
    hit = fit == FMAX
    assert 0 < hit.sum() < cc.N_POSES and (words[:, 3] != 0).any()
    assert np.array_equal((words != 0).any(axis=1), hit)


# ---------------------------------------------------------- 3. FAST against the float64 checker
@pytest.mark.parametrize("name", cc.NAMES)
def test_fast_against_the_float64_checker(runs, name):
    """Every pair of a node and a collider whose float64 gaps (Gottschalk's 15 axes on the float64 FK's boxes,
    tests/contacts_cases.py) decide its bit outside the band must have that bit.  The band: for the chains
    FAST decides by GJK (generic trees, the wide-angle masked chain) the project's stated sum, 3.5e-4 for
    GJK's touching tolerance + 2e-5 for FAST frame rounding = 3.7e-4; for the chains it decides by separating
    axes twice the largest |gap| at which a decision differed on an MI355X.
    Measured on an MI355X (600 poses per chain, 128400 pairs on the separating-axis chains): one decision
    differed from the checker's, on scene4, at |gap| = 7.1e-7 (scene6, serial20, masked: none), so the band is
    1.42e-6, which leaves 1 of 5803 near pairs of scene4 undecided and none elsewhere; on the GJK chains no
    decided pair differed, with 2 of 2335 (generic5), 2 of 6008 (masked_wide) and 0 of 579 (generic1) inside
    3.7e-4.
    At most 1% of the pairs that pass the sphere prefilter may fall inside the band."""
    chain, _, _ = cc.case(name)
    J = len(chain) - 1
    got = cc.unpack(runs[(name, "fast")]["words"], J)
    gn, gl, near = cc.sat_gaps(name)
    # the largest |gap| behind a differing decision, whatever the band: the pair's bit is the OR of its boxes,
    # so a set bit the checker has clear is explained by the nearer-to-touching box, a clear bit the checker
    # has set by the box that overlaps most
    h0 = (gn <= 0) | (gl <= 0)
    differ = h0 != got
    worst = float(np.where(got, np.minimum(gn, gl), -np.minimum(gn, gl))[differ].max()) if differ.any() else 0.0
    band = SAT_BAND if name in cc.SAT_ROUTE else cc.GJK_BAND
    hit, decided = cc.expected_bits(name, band)
    excluded = int((near & ~decided).sum())
    print(f"{name} fast: {int(differ.sum())} of {differ.size} pairs differ from the float64 checker, the largest "
          f"|gap| among them {worst:.3e}; band {band:.3e} leaves {excluded} of {int(near.sum())} near pairs undecided")
    assert excluded <= 0.01 * near.sum()
    assert np.array_equal(got[decided], hit[decided])


# --------------------------------------------------------------------- 4. pruning and indexing
@pytest.mark.parametrize("arith", ARITHS)
def test_pruned_colliders_keep_their_columns(device, arith):
    chain, boxes, _ = cc.case("scene4")
    far = boxes[1:2].copy()
    far["pos"] = (1000.0, 0.0, 0.0)
    x = dev(cc.poses("scene4"))
    with ikpso.BatchSolver(chain, 64, arith=arith, colliders=np.concatenate([boxes[0:1], far, boxes[2:3]])) as s:
        assert s.collider_count == 2
        three = s.contacts(x).cpu().numpy()
    with ikpso.BatchSolver(chain, 64, arith=arith, colliders=np.concatenate([boxes[0:1], boxes[2:3]])) as s:
        two = s.contacts(x).cpu().numpy()
    assert three.shape == (cc.N_POSES, 3) and two.shape == (cc.N_POSES, 2)
    assert (two[:, 0] != 0).any() and (two[:, 1] != 0).any()
    assert not three[:, 1].any()
    assert np.array_equal(three[:, [0, 2]], two)


@pytest.mark.parametrize("arith", ARITHS)
def test_nothing_within_reach(device, arith):
    chain, boxes, _ = cc.case("scene4")
    far = boxes.copy()
    far["pos"] += np.float32(1000.0)
    x = dev(cc.poses("scene4"))
    with ikpso.BatchSolver(chain, 64, arith=arith, colliders=far) as s:
        assert s.collider_count == 0
        words = torch.full((cc.N_POSES, 4), -1, dtype=torch.int32, device="cuda")
        pos = torch.empty((cc.N_POSES, 7, 3), dtype=torch.float32, device="cuda")
        fn = s._lib.ikpso_solver_evaluate_contacts
        assert fn(s._h, x.data_ptr(), cc.N_POSES, words.data_ptr(), pos.data_ptr(), None) == _abi.IKPSO_OK
        assert not words.any()
        assert torch.equal(pos, s.evaluate(x)[1])
    with ikpso.BatchSolver(chain, 64, arith=arith) as s:  # no colliders at all: C = 0, out_contacts may be NULL
        fn = s._lib.ikpso_solver_evaluate_contacts
        assert fn(s._h, x.data_ptr(), cc.N_POSES, None, pos.data_ptr(), None) == _abi.IKPSO_OK
        assert fn(s._h, x.data_ptr(), cc.N_POSES, None, None, None) == _abi.IKPSO_OK
        assert torch.equal(pos, s.evaluate(x)[1])
        w, p = s.contacts(x, positions=True)
        assert tuple(w.shape) == (cc.N_POSES, 0) and torch.equal(p, pos)


def test_argument_ladder(device):
    """With a solver: n < 0, NULL angles, then NULL out_contacts when the solver was given colliders, are
    IKPSO_ERR_INVALID_ARG; n == 0 is IKPSO_OK whatever the pointers."""
    x = dev(cc.poses("scene4"))
    with solver("scene4", "fast") as s:
        fn = s._lib.ikpso_solver_evaluate_contacts
        words = torch.zeros((cc.N_POSES, 4), dtype=torch.int32, device="cuda")
        bad = _abi.IKPSO_ERR_INVALID_ARG
        assert fn(s._h, x.data_ptr(), -1, words.data_ptr(), None, None) == bad
        assert fn(s._h, None, 4, words.data_ptr(), None, None) == bad
        assert fn(s._h, x.data_ptr(), 4, None, None, None) == bad
        assert fn(s._h, None, 0, None, None, None) == _abi.IKPSO_OK
        assert fn(s._h, x.data_ptr(), 1, words.data_ptr(), None, None) == _abi.IKPSO_OK
        one = s.contacts(x[:1])
        assert torch.equal(words[:1], one)  # one vector alone: the same words


# --------------------------------------------------------------------------------- 5. positions
@pytest.mark.parametrize("name,arith", params())
def test_positions_are_evaluates(runs, name, arith):
    r = runs[(name, arith)]
    d = float(np.max(np.abs(r["pos"].astype(np.float64) - r["epos"].astype(np.float64))))
    print(f"{name} {arith}: max |positions - evaluate's| = {d:.3e}")
    assert r["pos"].shape == r["epos"].shape
    if arith == "reference":
        assert np.array_equal(r["pos"].view(np.uint32), r["epos"].view(np.uint32))
    else:
        assert d <= FAST_POS_TOL


# ------------------------------------------------------------------------------- 6. the C example
def test_contacts_from_plain_c(device):
    b = subprocess.run(["make", "-C", str(EXAMPLES), "_build/contacts_c"], capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(EXAMPLES / "_build" / "contacts_c"), "8", "100"], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(l.startswith("answers: no contact") for l in lines)
    assert any(l.startswith("pushed: ") and "(node 1, collider 0)" in l for l in lines)
