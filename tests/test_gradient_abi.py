"""ikpso_solver_evaluate_gradient on the host side: the declaration, the symbol, the binding, the argument
checks that return before any device work, and the Python wrappers' shape checks (no solver is created
here, so nothing touches a device)."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ikpso
from ikpso import _abi

NAME = "ikpso_solver_evaluate_gradient"
HEADER = Path(__file__).resolve().parents[1] / "include" / "ikpso.h"
CTYPES = {"ikpso_solver*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
          "void*": ctypes.c_void_p, "int64_t": ctypes.c_int64}


def header_args():
    m = re.search(rf"ikpso_status {NAME}\(([^;]*)\);", HEADER.read_text())
    assert m, f"{NAME} not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry():
    assert header_args() == ["ikpso_solver* solver", "const float* angles", "const float* targets", "const float* rest",
                             "const float* target_rot", "const float* rot_weights", "int64_t n", "float* out_fitness",
                             "float* out_gradient", "void* stream"]
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
    fn = getattr(_abi.load(), NAME)
    assert fn(None, None, None, None, None, None, 0, None, None, None) == _abi.IKPSO_ERR_INVALID_ARG
    assert fn(None, None, None, None, None, None, -1, None, None, None) == _abi.IKPSO_ERR_INVALID_ARG


class _NoDeviceCall:
    """Stands in for the library: any entry the wrapper reaches fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached with bad shapes")


@pytest.mark.parametrize("method", ("gradient", "fitness"))
def test_wrappers_reject_bad_shapes_before_any_device_call(method):
    torch = pytest.importorskip("torch")
    s = object.__new__(ikpso.BatchSolver)
    s._lib, s._h = _NoDeviceCall(), None
    s.dof, s.effectors, s.chain = 21, 3, np.zeros(8, dtype=ikpso.NODE_DTYPE)
    call = getattr(s, method)

    def z(*shape):
        return torch.zeros(shape, dtype=torch.float32)

    with pytest.raises(ValueError, match="angles must be"):
        call(z(4, 20))
    with pytest.raises(ValueError, match="targets must be"):
        call(z(4, 21), targets=z(4, 2, 3))
    with pytest.raises(ValueError, match="rest must be"):
        call(z(4, 21), rest=z(3, 21))
    with pytest.raises(ValueError, match="effector_rot must be"):
        call(z(4, 21), effector_rot=z(4, 3, 9))
    with pytest.raises(ValueError, match="effector_rot_weight must"):
        call(z(4, 21), effector_rot=z(4, 3, 3, 3), effector_rot_weight=[1.0, 0.5])
    # a well-shaped host tensor stops at the tensor check, still before the library
    with pytest.raises(ValueError, match="must be on"):
        call(z(4, 21))
