"""ikpso_solve_batch_until on the host side: the symbol, its argument checks (which
return before any device work) and the host twin of the kernels' ordered_key."""
import ctypes
import math
import re
import subprocess

import numpy as np

from ikpso import _abi

NAME = "ikpso_solve_batch_until"


def test_symbol_exported_and_declared():
    assert NAME in _abi.SIGNATURES
    lib = _abi.load()
    assert hasattr(lib, NAME)
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(rf"\bT {NAME}$", nm, re.M)
    assert lib.ikpso_abi_version() == 5  # added after ABI 5: detected by symbol, the version stays


def test_null_solver_is_refused_without_device_work():
    lib = _abi.load()
    assert lib.ikpso_solve_batch_until(None, None, None, 1, 1, 0.5, None, None, None, None, None) == \
        _abi.IKPSO_ERR_INVALID_ARG


def test_nan_threshold_is_refused_without_device_work():
    lib = _abi.load()
    assert lib.ikpso_solve_batch_until(None, None, None, 1, 1, math.nan, None, None, None, None, None) == \
        _abi.IKPSO_ERR_INVALID_ARG
    # also with nothing to solve, where every other argument would pass
    assert lib.ikpso_solve_batch_until(None, None, None, 0, 0, math.nan, None, None, None, None, None) == \
        _abi.IKPSO_ERR_INVALID_ARG


def test_host_ordered_key_round_trips():
    """ordered_key_host (the threshold's key, computed on the host) against key_to_float:
    order-preserving, -0 canonicalised to +0, and no finite value or infinity maps to
    key 0, the value that disables the stop."""
    lib = _abi.load()
    key, back = lib.ikpso_debug_ordered_key, lib.ikpso_debug_key_to_float
    key.restype, key.argtypes = ctypes.c_uint32, [ctypes.c_float]
    back.restype, back.argtypes = ctypes.c_float, [ctypes.c_uint32]
    fmax = float(np.finfo(np.float32).max)
    vals = [-math.inf, -fmax, -1.0, -1e-30, -0.0, 0.0, 1e-45, 1e-30, 0.1, 1.0, fmax, math.inf]
    keys = [key(v) for v in vals]
    for v, k in zip(vals, keys):
        assert k != 0
        assert back(k) == float(np.float32(v))
        assert math.copysign(1.0, back(k)) == (1.0 if v == 0.0 else math.copysign(1.0, v))
    assert key(-0.0) == key(0.0) == 0x80000000
    assert keys[4] == keys[5] and keys[:5] == sorted(set(keys[:5])) and keys[5:] == sorted(set(keys[5:]))
    assert keys[3] < keys[4] < keys[6]
