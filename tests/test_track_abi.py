"""ikpso_solve_track on the host side: the symbol and the argument checks that return
before any device work (no solver is created here, so nothing touches a device)."""
import math
import re
import subprocess

from ikpso import _abi

NAME = "ikpso_solve_track"


def track(lib, solver=None, num_swarms=1, frames=1, max_iterations=1, stop=0.5):
    return lib.ikpso_solve_track(solver, None, None, num_swarms, frames, max_iterations, stop, None, None, None, None,
                                 None)


def test_symbol_exported_and_declared():
    assert NAME in _abi.SIGNATURES
    lib = _abi.load()
    assert hasattr(lib, NAME)
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(rf"\bT {NAME}$", nm, re.M)
    assert lib.ikpso_abi_version() == 5  # added after ABI 5: detected by symbol, the version stays


def test_null_solver_is_refused_without_device_work():
    lib = _abi.load()
    assert track(lib) == _abi.IKPSO_ERR_INVALID_ARG
    assert track(lib, frames=0) == _abi.IKPSO_ERR_INVALID_ARG


def test_nan_threshold_is_refused_without_device_work():
    lib = _abi.load()
    assert track(lib, stop=math.nan) == _abi.IKPSO_ERR_INVALID_ARG
    # also with nothing to solve, where every other argument would pass
    assert track(lib, frames=0, stop=math.nan) == _abi.IKPSO_ERR_INVALID_ARG
    assert track(lib, num_swarms=0, frames=0, max_iterations=0, stop=math.nan) == _abi.IKPSO_ERR_INVALID_ARG


def test_negative_frames_are_refused_without_device_work():
    lib = _abi.load()
    assert track(lib, frames=-1) == _abi.IKPSO_ERR_INVALID_ARG
    assert track(lib, num_swarms=0, frames=-1) == _abi.IKPSO_ERR_INVALID_ARG
