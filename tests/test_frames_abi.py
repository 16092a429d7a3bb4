"""ikpso_solve_track_frames on the host side: the declaration, the symbol, the binding and the
argument checks that return before any device work (no solver is created here, so nothing touches a
device)."""
import ctypes
import math
import re
import subprocess
from pathlib import Path

from ikpso import _abi

NAME = "ikpso_solve_track_frames"
HEADER = Path(__file__).resolve().parents[1] / "include" / "ikpso.h"


def test_header_declares_the_entry():
    text = HEADER.read_text()
    m = re.search(rf"ikpso_status {NAME}\(([^;]*)\);", text)
    assert m, f"{NAME} not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["ikpso_solver* solver", "const float* targets", "const float* target_rot",
                    "const float* rot_weights", "const float* start_pose", "int64_t num_swarms", "int32_t frames",
                    "int32_t max_iterations", "float stop_fitness", "float* out_angles", "float* out_fitness",
                    "float* out_residual", "int32_t* out_iterations", "void* stream"]
    assert re.search(r"#define IKPSO_ABI_VERSION 5\b", text)


def test_symbol_exported_and_bound():
    vp, f, i32, i64 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int32, ctypes.c_int64
    assert _abi.SIGNATURES[NAME] == (i32, [vp, vp, vp, vp, vp, i64, i32, i32, f, vp, vp, vp, vp, vp])
    lib = _abi.load()
    fn = getattr(lib, NAME)
    assert fn.restype is i32 and list(fn.argtypes) == _abi.SIGNATURES[NAME][1]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(rf"\bT {NAME}$", nm, re.M)
    assert lib.ikpso_abi_version() == 5  # added after ABI 5: detected by symbol, the version stays


def frames(lib, solver=None, num_swarms=1, frames=1, max_iterations=1, stop=0.5):
    return getattr(lib, NAME)(solver, None, None, None, None, num_swarms, frames, max_iterations, stop, None, None,
                              None, None, None)


def test_null_solver_and_nan_threshold_are_refused_without_device_work():
    lib = _abi.load()
    assert frames(lib) == _abi.IKPSO_ERR_INVALID_ARG
    assert frames(lib, frames=0) == _abi.IKPSO_ERR_INVALID_ARG
    assert frames(lib, num_swarms=0, frames=0, max_iterations=0, stop=math.nan) == _abi.IKPSO_ERR_INVALID_ARG
    assert frames(lib, frames=-1) == _abi.IKPSO_ERR_INVALID_ARG
