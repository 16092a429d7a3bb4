"""ikpso_solver_evaluate_frames on the host side: the declaration, the symbol, the binding, the
argument checks that return before any device work, and the Python wrapper's shape checks (no solver
is created here, so nothing touches a device)."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ikpso
from ikpso import _abi

NAME = "ikpso_solver_evaluate_frames"
HEADER = Path(__file__).resolve().parents[1] / "include" / "ikpso.h"


def test_header_declares_the_entry():
    text = HEADER.read_text()
    m = re.search(rf"ikpso_status {NAME}\(([^;]*)\);", text)
    assert m, f"{NAME} not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["ikpso_solver* solver", "const float* angles", "const float* targets", "const float* rest",
                    "const float* target_rot", "const float* rot_weights", "int64_t n", "float* out_fitness",
                    "float* out_positions", "float* out_rotations", "float* out_rot_error", "void* stream"]
    assert re.search(r"#define IKPSO_ABI_VERSION 5\b", text)


def test_symbol_exported_and_bound():
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert _abi.SIGNATURES[NAME] == (i32, [vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp])
    lib = _abi.load()
    fn = getattr(lib, NAME)
    assert fn.restype is i32 and list(fn.argtypes) == _abi.SIGNATURES[NAME][1]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(rf"\bT {NAME}$", nm, re.M)
    assert lib.ikpso_abi_version() == 5  # added after ABI 5: detected by symbol, the version stays


def test_null_solver_and_negative_n_are_refused_without_device_work():
    fn = getattr(_abi.load(), NAME)
    assert fn(None, None, None, None, None, None, 0, None, None, None, None, None) == _abi.IKPSO_ERR_INVALID_ARG
    assert fn(None, None, None, None, None, None, -1, None, None, None, None, None) == _abi.IKPSO_ERR_INVALID_ARG


class _NoDeviceCall:
    """Stands in for the library: any entry the wrapper reaches fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached with bad shapes")


def _shell(dof=21, effectors=3, nodes=8):
    """A BatchSolver without a handle: the attributes the wrapper's shape checks read."""
    s = object.__new__(ikpso.BatchSolver)
    s._lib, s._h = _NoDeviceCall(), None
    s.dof, s.effectors, s.chain = dof, effectors, np.zeros(nodes, dtype=ikpso.NODE_DTYPE)
    return s


def test_wrapper_rejects_bad_shapes_before_any_device_call():
    torch = pytest.importorskip("torch")
    s, n = _shell(), 4
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32)  # noqa: E731
    cases = {
        "angles": dict(angles=z(n, 20)),
        "targets": dict(angles=z(n, 21), targets=z(n, 2, 3)),
        "rest": dict(angles=z(n, 21), rest=z(n + 1, 21)),
        "effector_rot must": dict(angles=z(n, 21), effector_rot=z(n, 3, 9)),
        "effector_rot_weight": dict(angles=z(n, 21), effector_rot=z(n, 3, 3, 3), effector_rot_weight=[1.0, 2.0]),
    }
    for what, kw in cases.items():
        with pytest.raises(ValueError, match=what):
            s.evaluate_frames(**kw)
    # well-shaped host tensors stop at the tensor check, still before the library
    with pytest.raises(ValueError, match="must be on"):
        s.evaluate_frames(z(n, 21), z(n, 3, 3), z(n, 21), z(n, 3, 3, 3), 1.0)


def test_rotation_angle():
    theta = np.array([0.0, 1e-3, 0.5, np.pi / 2, 3.0, np.pi])
    e = 4.0 * (1.0 - np.cos(theta))
    assert np.allclose(ikpso.rotation_angle(e), theta, rtol=0, atol=1e-9)
    assert np.array_equal(ikpso.rotation_angle(np.array([-1e-7, 8.0 + 1e-6])), [0.0, np.pi])  # clipped, never NaN
    torch = pytest.importorskip("torch")
    got = ikpso.rotation_angle(torch.from_numpy(e))
    assert isinstance(got, torch.Tensor) and np.allclose(got.numpy(), theta, rtol=0, atol=1e-9)
