"""ikpso_solver_evaluate_contacts on the host side: the declaration, the symbol, the binding, the argument
checks that return before any device work, the decoding helpers, and -- with the oracle and the float64
checker alone -- that the chains of tests/test_gpu_contacts.py exercise both outcomes and keep the checker's
undecided band small (no solver is created here, so nothing touches a device)."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import contacts_cases as cc
import ikpso
from ikpso import _abi

NAME = "ikpso_solver_evaluate_contacts"
HEADER = Path(__file__).resolve().parents[1] / "include" / "ikpso.h"
CTYPES = {"ikpso_solver*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
          "uint32_t*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int64_t": ctypes.c_int64}


def header_args():
    m = re.search(rf"ikpso_status {NAME}\(([^;]*)\);", HEADER.read_text())
    assert m, f"{NAME} not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry():
    assert header_args() == ["ikpso_solver* solver", "const float* angles", "int64_t n", "uint32_t* out_contacts",
                             "float* out_positions", "void* stream"]
    assert re.search(r"#define IKPSO_ABI_VERSION 5\b", HEADER.read_text())


def test_binding_has_the_headers_argument_list():
    restype, argtypes = _abi.SIGNATURES[NAME]
    assert restype is ctypes.c_int32
    assert argtypes == [CTYPES[a.rsplit(" ", 1)[0]] for a in header_args()]


def test_symbol_exported_and_bound():
    lib = _abi.load()
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int32 and list(fn.argtypes) == _abi.SIGNATURES[NAME][1]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(rf"\bT {NAME}$", nm, re.M)
    assert lib.ikpso_abi_version() == 5  # added after ABI 5: detected by symbol, the version stays


def test_null_solver_and_negative_n_are_refused_without_device_work():
    """The first rungs of the documented order: a NULL solver whatever else is given, then n < 0.  (The NULL
    angles and NULL out_contacts rungs need a solver: tests/test_gpu_contacts.py.)"""
    fn = getattr(_abi.load(), NAME)
    assert fn(None, None, 0, None, None, None) == _abi.IKPSO_ERR_INVALID_ARG
    assert fn(None, None, -1, None, None, None) == _abi.IKPSO_ERR_INVALID_ARG
    assert fn(None, None, 4, None, None, None) == _abi.IKPSO_ERR_INVALID_ARG


class _NoDeviceCall:
    """Stands in for the library: any entry the wrapper reaches fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached with bad shapes")


def test_wrapper_rejects_bad_shapes_before_any_device_call():
    torch = pytest.importorskip("torch")
    s = object.__new__(ikpso.BatchSolver)
    s._lib, s._h = _NoDeviceCall(), None
    s.dof, s.effectors, s.chain, s.colliders_given = 21, 3, np.zeros(8, dtype=ikpso.NODE_DTYPE), 4
    with pytest.raises(ValueError, match="angles must be"):
        s.contacts(torch.zeros((4, 20), dtype=torch.float32))
    # a well-shaped host tensor stops at the tensor check, still before the library
    with pytest.raises(ValueError, match="must be on"):
        s.contacts(torch.zeros((4, 21), dtype=torch.float32), positions=True)


def test_contact_nodes_decodes_a_word():
    assert ikpso.contact_nodes(0) == []
    assert ikpso.contact_nodes(1) == [1]                      # bit 0: node 1
    assert ikpso.contact_nodes(1 << 19) == [20]               # bit 19: the 20th node
    assert ikpso.contact_nodes((1 << 19) | 0b101) == [1, 3, 20]
    assert ikpso.contact_nodes(np.int32(-2**31)) == [32]      # an int32 word with its top bit set
    assert ikpso.contact_nodes(np.uint32(0x80000001)) == [1, 32]


def test_contact_pairs_lists_pose_collider_node():
    words = np.array([[0, 1], [1 << 19, 0], [0, 0], [0b110, (1 << 19) | 1]], dtype=np.uint32)
    want = [(0, 1, 1), (1, 0, 20), (3, 0, 2), (3, 0, 3), (3, 1, 1), (3, 1, 20)]
    for w in (words, words.view(np.int32)):
        got = ikpso.contact_pairs(w)
        assert got.dtype == np.int64 and got.shape == (6, 3)
        assert [tuple(r) for r in got.tolist()] == want
    assert ikpso.contact_pairs(np.zeros((3, 2), dtype=np.int32)).shape == (0, 3)
    assert ikpso.contact_pairs(np.zeros((3, 0), dtype=np.int32)).shape == (0, 3)
    torch = pytest.importorskip("torch")
    assert [tuple(r) for r in ikpso.contact_pairs(torch.from_numpy(words.view(np.int32))).tolist()] == want
    with pytest.raises(ValueError):
        ikpso.contact_pairs(np.zeros(4, dtype=np.int32))


@pytest.mark.parametrize("name", cc.NAMES)
def test_cases_exercise_both_outcomes_and_the_checker_agrees_with_the_oracle(oracle, name):
    """What the GPU tests rest on, held on the CPU: per chain the share of colliding poses lies in (0.05,
    0.95); the 20-joint chain sets bit 19; the float64 separating-axis checker and the oracle's GJK agree on
    every pair the checker decides at the GJK band; and that band leaves at most 1% of the pairs that pass
    the sphere prefilter undecided."""
    chain, boxes, _ = cc.case(name)
    J = len(chain) - 1
    bits = cc.oracle_bits(oracle, name)
    assert bits.shape == (cc.N_POSES, len(boxes))
    assert 0.05 < (bits != 0).any(axis=1).mean() < 0.95
    got = cc.unpack(bits, J)
    if name == "serial20":
        assert got[:, 19, :].any()
    assert not (bits >> np.uint32(J)).any()
    hit, decided = cc.expected_bits(name, cc.GJK_BAND)
    assert np.array_equal(hit[decided], got[decided])
    near = cc.sat_gaps(name)[2]
    assert (near & ~decided).sum() <= 0.01 * near.sum()
