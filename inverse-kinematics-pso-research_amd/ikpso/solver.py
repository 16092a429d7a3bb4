"""Python mirror of the reference's solver interface over the C ABI.

Reference entry points (src/ = InverseKinematicsResearch/InverseKinematicsResearch/):
    initGenerators(curandState_t* randoms, int size)        src/utility_kernels.cuh:33-47
    calculatePSO(particles, positions, bests, randoms, size, chain, PSOConfig,
                 FitnessConfig, Coordinates* result, obj_t* colliders,
                 int colliderCount)                          src/kernel.cu:279-327
Both return a status code (cudaError_t there, ikpso_status here: 0 = success,
anything else = the caller's frame loop aborts, src/Main.cpp:225-226).

Device buffers are torch tensors on a ROCm device (torch is plumbing for
device memory and streams); host-side buffers may be numpy arrays.  The
batched API (``BatchSolver``) is the MI355X-native extension: B independent
swarms per call, one kernel launch.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _abi
from ._abi import NODE_DTYPE, RNG_WORDS, FitnessConfig as _CFit, PSOConfig as _CPso, SolverDesc


@dataclass
class PSOConfig:
    """PSOConfig (src/Particle.h:70-85); defaults are the struct's own.
    The visualiser uses PSOConfig(0.5, 0.5, 1.25, 15) (src/Main.cpp:130)."""

    inertia: float = 0.2
    local: float = 0.5
    global_: float = 0.7
    iterations: int = 10

    def c(self) -> _CPso:
        return _CPso(self.inertia, self.local, self.global_, int(self.iterations))


@dataclass
class FitnessConfig:
    """FitnessConfig (src/Particle.h:55-68); the visualiser uses (3, 0, 0.1)."""

    angle_weight: float = 3.0
    distance_weight: float = 0.0
    error_threshold: float = 0.1

    def c(self) -> _CFit:
        return _CFit(self.angle_weight, self.distance_weight, self.error_threshold)


MAIN_PSO = PSOConfig(0.5, 0.5, 1.25, 15)       # src/Main.cpp:130
MAIN_FITNESS = FitnessConfig(3.0, 0.0, 0.1)    # src/Main.cpp:131


def _torch():
    import torch

    return torch


def _dev_ptr(t) -> Optional[int]:
    """Device pointer of a torch tensor (must be on a GPU and contiguous)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("expected a device tensor")
    if not t.is_contiguous():
        raise ValueError("expected a contiguous tensor")
    return t.data_ptr()


def _any_ptr(x, keep: list) -> Optional[int]:
    """Pointer to host (numpy) or device (torch) memory."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        keep.append(a)
        return a.ctypes.data
    if x.is_cuda:
        return _dev_ptr(x)
    if not x.is_contiguous():
        x = x.contiguous()
    keep.append(x)
    return x.data_ptr()


def _stream_handle(stream) -> Optional[int]:
    torch = _torch()
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream or None


def _colliders(colliders) -> np.ndarray:
    """obj_t array (COLLIDER_DTYPE) from a compatible numpy array."""
    b = np.ascontiguousarray(colliders)
    if b.dtype != _abi.COLLIDER_DTYPE:
        if b.dtype.itemsize != _abi.COLLIDER_DTYPE.itemsize:
            raise TypeError("colliders must be an obj_t (COLLIDER_DTYPE) array")
        b = b.view(_abi.COLLIDER_DTYPE)
    return b.reshape(-1)


def make_collider(size, pos, quat=(0.0, 0.0, 0.0, 1.0)) -> np.ndarray:
    """One obj_t: size = (x, y, z) box edge lengths, pos = centre, quat = (x, y, z, w)."""
    c = np.zeros(1, dtype=_abi.COLLIDER_DTYPE)
    c["x"], c["y"], c["z"] = size
    c["pos"] = pos
    c["quat"] = quat
    return c


def rotation_angle(rot_error):
    """Geodesic angle (radians) between two rotations from their squared Frobenius distance
    |Ra - Rb|_F^2 = 4 (1 - cos theta) -- BatchSolver.evaluate_frames' rot_error: arccos(clip(1 - e / 4,
    -1, 1)).  A torch tensor gives a tensor, anything else a numpy array."""
    if hasattr(rot_error, "clamp"):
        return (1.0 - rot_error / 4.0).clamp(-1.0, 1.0).acos()
    return np.arccos(np.clip(1.0 - np.asarray(rot_error) / 4.0, -1.0, 1.0))


def manipulability(jac, rows=slice(0, 3)) -> np.ndarray:
    """Yoshikawa's manipulability sqrt(det(J J^T)) over the chosen rows of BatchSolver.jacobian's [..., 6, D]
    Jacobians (rows 0..2 linear, the default; 3..5 angular; slice(0, 6) both), in numpy float64: [...].  0 at a
    singularity of those rows, and wherever D is smaller than their number."""
    j = jac.detach().cpu().numpy() if hasattr(jac, "detach") else np.asarray(jac)
    j = j.astype(np.float64)[..., rows, :]
    return np.sqrt(np.maximum(np.linalg.det(j @ np.swapaxes(j, -1, -2)), 0.0))


def contact_nodes(word) -> list:
    """The node indices k (1 .. 32, ascending) whose bit k - 1 is set in one word of BatchSolver.contacts()."""
    w = int(word) & 0xFFFFFFFF
    return [k for k in range(1, 33) if (w >> (k - 1)) & 1]


def contact_pairs(contacts) -> np.ndarray:
    """Every contact of BatchSolver.contacts()' [n, C] words (a tensor or an array) as an int64 array [m, 3] of
    (pose, collider, node) rows, sorted by pose, then collider, then node; node is the 1-based node index."""
    c = contacts.detach().cpu().numpy() if hasattr(contacts, "detach") else np.asarray(contacts)
    if c.ndim != 2:
        raise ValueError("contacts must be [n, C]")
    bits = (c.astype(np.int64)[:, :, None] >> np.arange(32, dtype=np.int64)) & 1
    pose, coll, node = np.nonzero(bits)
    return np.stack([pose, coll, node + 1], axis=1).astype(np.int64)


def rng_tensor(count: int, device="cuda"):
    """Device buffer for `count` generator states (48 bytes each, curandState_t layout)."""
    torch = _torch()
    return torch.zeros((count, RNG_WORDS), dtype=torch.int32, device=device)


def particles_tensor(size: int, dof: int, device="cuda"):
    """Device buffer for the reference's particles array: [3][dof][size] floats."""
    torch = _torch()
    return torch.zeros((3, dof, size), dtype=torch.float32, device=device)


def init_generators(randoms, size: int, stream=None) -> int:
    """initGenerators: randoms[i] = curand_init(i, 0, 0).  Returns the status."""
    lib = _abi.load()
    return lib.ikpso_init_generators(_dev_ptr(randoms), int(size), _stream_handle(stream))


def init_generators_seeded(randoms, count: int, seed_base: int, stream=None) -> int:
    lib = _abi.load()
    return lib.ikpso_init_generators_seeded(_dev_ptr(randoms), int(count), int(seed_base), _stream_handle(stream))


def calculate_pso(particles, positions, bests, randoms, size: int, chain: np.ndarray, pso_config: PSOConfig,
                  fit_config: FitnessConfig, result, colliders=None, collider_count: int = 0, stream=None) -> int:
    """calculatePSO over the C ABI; same arguments, same meaning, same status
    convention.  `chain` is a NODE_DTYPE array (host) or device tensor;
    `result` receives the global-best angles (numpy array or tensor);
    `colliders` an obj_t array (numpy COLLIDER_DTYPE or a device tensor) with
    `collider_count` entries (src/kernel.cu:104-136)."""
    lib = _abi.load()
    keep: list = []
    if isinstance(colliders, np.ndarray):
        colliders = _colliders(colliders)
    if isinstance(chain, np.ndarray):
        if chain.dtype != NODE_DTYPE:
            raise TypeError("chain must be an ikpso NODE_DTYPE array")
        node_count = int(chain.shape[0])
    else:
        node_count = int(chain.numel() * chain.element_size() // NODE_DTYPE.itemsize)
    return lib.ikpso_calculate_pso(
        _dev_ptr(particles), _any_ptr(positions, keep), _dev_ptr(bests), _dev_ptr(randoms), int(size),
        _any_ptr(chain, keep), node_count, pso_config.c(), fit_config.c(), _any_ptr(result, keep),
        _any_ptr(colliders, keep), int(collider_count), _stream_handle(stream))


class BatchSolver:
    """B independent swarms (IK targets) per call over one shared chain.

    RNG streams are owned by the solver and persist across calls (like the
    reference's randoms buffer); local swarm b of a solver seeded with
    first_swarm = f draws the streams curand_init(seed_base + (f + b) * P + i).
    """

    def __init__(self, chain: np.ndarray, particles: int, pso: PSOConfig = MAIN_PSO,
                 fit: FitnessConfig = MAIN_FITNESS, arith: str = "fast", positions=None,
                 limit_weight: float = 0.0, soft_lo=None, soft_hi=None, kernel: str = "auto", colliders=None,
                 posref_node_slot: bool = False, axis_mask=None, fold: bool = True):
        self._lib = _abi.load()
        if chain.dtype != NODE_DTYPE:
            raise TypeError("chain must be an ikpso NODE_DTYPE array")
        self.chain = np.ascontiguousarray(chain)
        self.P = int(particles)
        self.pso = pso
        self.fit = fit
        keep: list = []
        desc = SolverDesc()
        desc.chain = self.chain.ctypes.data
        desc.node_count = self.chain.shape[0]
        desc.particles = self.P
        desc.pso = pso.c()
        desc.fit = fit.c()
        desc.arith = {"fast": _abi.ARITH_FAST, "reference": _abi.ARITH_REFERENCE}[arith]
        desc.kernel = {"auto": _abi.KERNEL_AUTO, "resident": _abi.KERNEL_RESIDENT,
                       "streaming": _abi.KERNEL_STREAMING, "coop": _abi.KERNEL_COOP}[kernel]
        desc.positions = _any_ptr(None if positions is None else np.asarray(positions, np.float32), keep)
        desc.limit_weight = float(limit_weight)
        desc.soft_lo = _any_ptr(None if soft_lo is None else np.asarray(soft_lo, np.float32), keep)
        desc.soft_hi = _any_ptr(None if soft_hi is None else np.asarray(soft_hi, np.float32), keep)
        desc.flags = (_abi.FLAG_POSREF_NODE_SLOT if posref_node_slot else 0) | (0 if fold else _abi.FLAG_NO_FOLD)
        if axis_mask is not None:  # [node_count] uint8: bit c = Euler angle c of node k is free
            m = np.ascontiguousarray(axis_mask, dtype=np.uint8)
            if m.shape != (self.chain.shape[0],):
                raise ValueError(f"axis_mask must have one entry per node ({self.chain.shape[0]})")
            desc.axis_mask = _any_ptr(m, keep)
        self.axis_mask = None if axis_mask is None else np.array(axis_mask, dtype=np.uint8)
        if colliders is not None and len(colliders):
            boxes = _colliders(colliders)
            desc.colliders = _any_ptr(boxes, keep)
            desc.collider_count = int(boxes.shape[0])
        self.colliders_given = int(desc.collider_count)  # the columns of contacts()
        handle = ctypes.c_void_p()
        _abi.check(self._lib.ikpso_solver_create(ctypes.byref(desc), ctypes.byref(handle)), "ikpso_solver_create")
        self._h = handle
        self.dof = self._lib.ikpso_solver_dof(self._h)
        self.effectors = self._lib.ikpso_solver_effectors(self._h)
        self.capacity = 0
        self._seeded_on = None

    @property
    def collider_count(self) -> int:
        """Colliders the kernels test (0 when none is within the arm's reach)."""
        return self._lib.ikpso_solver_collider_count(self._h)

    @property
    def kernel(self) -> str:
        """Kernel variant the solver dispatches to (the last solve's, once one ran)."""
        return self._lib.ikpso_solver_kernel_name(self._h).decode()

    def seed(self, capacity: int, seed_base: int = 0, first_swarm: int = 0, stream=None) -> None:
        torch = _torch()
        _abi.check(self._lib.ikpso_solver_seed(self._h, int(capacity), int(seed_base), int(first_swarm),
                                               _stream_handle(stream)), "ikpso_solver_seed")
        self._seeded_on = torch.device("cuda", torch.cuda.current_device())  # where the generator states live
        self.capacity = max(self.capacity, int(capacity))

    def _check_tensor(self, t, name: str, device) -> None:
        """float32, contiguous, on the solver's device (the kernels read raw fp32)."""
        torch = _torch()
        if t is None:
            return
        if not t.is_cuda or t.device != device:
            raise ValueError(f"{name} must be on {device}, got {t.device}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")

    def solve(self, targets=None, start_pose=None, iterations: Optional[int] = None, num_swarms: Optional[int] = None,
              out: Optional[Tuple] = None, residual: bool = True, stream=None, sync: bool = True):
        """targets: device [B, E, 3] (None: chain targets); start_pose: device [B, D] or None.
        Returns (angles [B, D], fitness [B], residual [B] or None) device tensors.
        sync: settle a cooperative-family solve before returning (ikpso_solver_sync:
        waits for it, and re-runs it on the streaming kernels if the GPU's other work
        kept a group from assembling); no effect on the other families, which stay
        stream-ordered and asynchronous."""
        torch = _torch()
        if num_swarms is None:
            if targets is None:
                raise ValueError("num_swarms is required when targets is None")
            num_swarms = int(targets.shape[0])
        B = int(num_swarms)
        it = self.pso.iterations if iterations is None else int(iterations)
        if targets is not None and tuple(targets.shape) != (B, self.effectors, 3):
            raise ValueError(f"targets must be [{B}, {self.effectors}, 3]")
        if start_pose is not None and tuple(start_pose.shape) != (B, self.dof):
            raise ValueError(f"start_pose must be [{B}, {self.dof}]")
        dev = self._device()
        if out is None:
            angles = torch.empty((B, self.dof), dtype=torch.float32, device=dev)
            fitness = torch.empty((B,), dtype=torch.float32, device=dev)
            res = torch.empty((B,), dtype=torch.float32, device=dev) if residual else None
        else:
            angles, fitness, res = out
            if tuple(angles.shape) != (B, self.dof) or tuple(fitness.shape) != (B,) or (
                    res is not None and tuple(res.shape) != (B,)):
                raise ValueError("out must be ([B, D], [B], [B] or None)")
        for t, name in ((targets, "targets"), (start_pose, "start_pose"), (angles, "out angles"),
                        (fitness, "out fitness"), (res, "out residual")):
            self._check_tensor(t, name, dev)
        _abi.check(self._lib.ikpso_solve_batch(self._h, _dev_ptr(targets), _dev_ptr(start_pose), B, it,
                                               _dev_ptr(angles), _dev_ptr(fitness), _dev_ptr(res),
                                               _stream_handle(stream)), "ikpso_solve_batch")
        if sync:
            _abi.check(self._lib.ikpso_solver_sync(self._h), "ikpso_solver_sync")
        return angles, fitness, res

    def _device(self):
        """Where the generator states live (seed()); before any, the current device."""
        torch = _torch()
        return self._seeded_on or torch.device("cuda", torch.cuda.current_device())

    def _outputs(self, shape: Tuple[int, ...], residual: bool, dev):
        """(angles [*shape, D], fitness [*shape], residual [*shape] or None, iterations [*shape] int32)"""
        torch = _torch()
        return (torch.empty(shape + (self.dof,), dtype=torch.float32, device=dev),
                torch.empty(shape, dtype=torch.float32, device=dev),
                torch.empty(shape, dtype=torch.float32, device=dev) if residual else None,
                torch.empty(shape, dtype=torch.int32, device=dev))

    def _host_weights(self, effector_rot_weight):
        """effector_rot_weight (a scalar or E values) as the E host floats an entry reads during the call;
        None (every weight 0) stays None."""
        if effector_rot_weight is None:
            return None
        E = self.effectors
        w = np.asarray(effector_rot_weight, dtype=np.float32).reshape(-1)
        if w.size == 1:
            w = np.repeat(w, E)
        if w.shape != (E,):
            raise ValueError(f"effector_rot_weight must be a scalar or hold {E} values")
        return (ctypes.c_float * E)(*w.tolist())

    @staticmethod
    def _term_form(target_rot, orientation_weight, aim_dir, aim_axis, aim_weight, effector_rot, effector_rot_weight):
        """The form the term arguments of solve_until / solve_track select, as (name, the form's device
        tensor, its host arguments); (None, None, None) for the plain call."""
        if target_rot is not None and aim_dir is not None:
            raise ValueError("target_rot and aim_dir are not combined: pass one or the other")
        frames_form = effector_rot is not None or effector_rot_weight is not None
        if frames_form and (target_rot is not None or aim_dir is not None):
            raise ValueError("effector_rot is not combined with target_rot or aim_dir: pass one or the other")
        if target_rot is not None:
            return "pose", target_rot, orientation_weight
        if aim_dir is not None:
            return "aim", aim_dir, (aim_axis, aim_weight)
        if frames_form:
            return "effector_rot", effector_rot, effector_rot_weight
        return None, None, None

    def _solve_form(self, form, targets, start_pose, B: int, T: int, it: int, stop: float, outs, stream) -> None:
        """ikpso_solve_track, or the entry of `form` (_term_form), over time-major buffers.  "pose": T * B
        row-major 3x3 rotations of the effector node's frame, and the weight.  "aim": T * B world
        directions, and (the tool axis in the effector node's frame, 3 host values; the weight).
        "effector_rot": T * B * E row-major 3x3 rotations (or None with every weight 0), and one weight or
        E of them (host)."""
        name, extra, host = form
        E = self.effectors
        if name == "pose":
            if extra.numel() != T * B * 9 or tuple(extra.shape[-2:]) != (3, 3):
                raise ValueError(f"target_rot must hold {T * B} rotations [..., 3, 3]")
            entry, tensor, term = "ikpso_solve_track_pose", "target_rot", lambda p: (p, float(host))
        elif name == "aim":
            if extra.numel() != T * B * 3 or int(extra.shape[-1]) != 3:
                raise ValueError(f"aim_dir must hold {T * B} directions [..., 3]")
            axis = np.asarray(host[0], dtype=np.float32).reshape(-1)
            if axis.shape != (3,):
                raise ValueError("aim_axis must hold 3 values")
            host_axis = (ctypes.c_float * 3)(*axis.tolist())  # read during the call
            entry, tensor, term = "ikpso_solve_track_aim", "aim_dir", lambda p: (p, host_axis, float(host[1]))
        elif name == "effector_rot":
            if extra is not None and (extra.numel() != T * B * E * 9 or tuple(extra.shape[-2:]) != (3, 3)):
                raise ValueError(f"effector_rot must hold {T * B * E} rotations [..., {E}, 3, 3]")
            host_w = self._host_weights(host)
            entry, tensor, term = "ikpso_solve_track_frames", "effector_rot", lambda p: (p, host_w)
        else:
            entry, tensor, term = "ikpso_solve_track", "", lambda p: ()
        for t, tname in ((targets, "targets"), (start_pose, "start_pose"), (extra, tensor)):
            self._check_tensor(t, tname, self._device())
        _abi.check(getattr(self._lib, entry)(self._h, _dev_ptr(targets), *term(_dev_ptr(extra)), _dev_ptr(start_pose),
                                             B, T, it, stop, *(_dev_ptr(o) for o in outs), _stream_handle(stream)),
                   entry)

    def solve_until(self, targets=None, start_pose=None, max_iterations: Optional[int] = None,
                    stop_fitness: Optional[float] = None, num_swarms: Optional[int] = None, residual: bool = True,
                    stream=None, target_rot=None, orientation_weight: float = 0.0, aim_dir=None,
                    aim_axis=(0.0, 0.0, 1.0), aim_weight: float = 0.0, effector_rot=None, effector_rot_weight=None):
        """solve() with a per-swarm early stop (ikpso_solve_batch_until): swarm b stops after the
        first iteration n >= 0 at which its global-best fitness is <= stop_fitness, else it runs
        max_iterations (None: the solver's PSOConfig.iterations).  stop_fitness tests the fitness,
        not the residual; None takes the solver's FitnessConfig.error_threshold, a negative value
        never stops.  Returns (angles [B, D], fitness [B], residual [B] or None, iterations [B]
        int32) device tensors; a stopped swarm's answers and generator states are those of
        solve(iterations=n), bit for bit.  Runs the resident or the streaming kernels; a
        kernel="coop" solver raises (unsupported configuration).  Stream-ordered, asynchronous.
        target_rot (device [B, 3, 3] float32) with orientation_weight: the pose form, one frame of
        solve_track's (see there); it needs targets.  aim_dir (device [B, 3] float32) with aim_axis
        and aim_weight: the aim form, likewise; not together with target_rot.  effector_rot (device
        [B, E, 3, 3] float32) with effector_rot_weight: per-effector orientation targets of an unmasked
        Euler chain or tree, one frame of solve_track's; not together with either."""
        form = self._term_form(target_rot, orientation_weight, aim_dir, aim_axis, aim_weight, effector_rot,
                               effector_rot_weight)
        if num_swarms is None:
            if targets is None:
                raise ValueError("num_swarms is required when targets is None")
            num_swarms = int(targets.shape[0])
        B = int(num_swarms)
        it = self.pso.iterations if max_iterations is None else int(max_iterations)
        stop = self.fit.error_threshold if stop_fitness is None else float(stop_fitness)
        if targets is not None and tuple(targets.shape) != (B, self.effectors, 3):
            raise ValueError(f"targets must be [{B}, {self.effectors}, 3]")
        if start_pose is not None and tuple(start_pose.shape) != (B, self.dof):
            raise ValueError(f"start_pose must be [{B}, {self.dof}]")
        dev = self._device()
        outs = angles, fitness, res, iters = self._outputs((B,), residual, dev)
        if form[0] is not None:
            if targets is None:
                raise ValueError(f"the {form[0]} form needs targets")
            self._solve_form(form, targets, start_pose, B, 1, it, stop, outs, stream)
            return outs
        for t, name in ((targets, "targets"), (start_pose, "start_pose")):
            self._check_tensor(t, name, dev)
        _abi.check(self._lib.ikpso_solve_batch_until(self._h, _dev_ptr(targets), _dev_ptr(start_pose), B, it, stop,
                                                     _dev_ptr(angles), _dev_ptr(fitness), _dev_ptr(res),
                                                     _dev_ptr(iters), _stream_handle(stream)),
                   "ikpso_solve_batch_until")
        return outs

    def solve_track(self, targets, start_pose=None, iterations: Optional[int] = None,
                    stop_fitness: Optional[float] = None, residual: bool = True, stream=None, target_rot=None,
                    orientation_weight: float = 0.0, aim_dir=None, aim_axis=(0.0, 0.0, 1.0), aim_weight: float = 0.0,
                    effector_rot=None, effector_rot_weight=None):
        """B swarms following T waypoints each (ikpso_solve_track): targets is device [T, B, E, 3],
        time-major; frame t of swarm b is solve_until on targets[t] with `iterations` as its
        maximum (None: the solver's PSOConfig.iterations), warm-started from start_pose (device
        [B, D] or None: the chain rotations) for t = 0 and from frame t-1's answer after that, bit
        for bit -- outputs, iteration counts and the generator states left in the solver.  Every
        frame is a fresh swarm; only the generators carry on.  stop_fitness=None never stops.
        Returns (angles [T, B, D], fitness [T, B], residual [T, B] or None, iterations [T, B]
        int32) device tensors.  The resident family runs the whole track in one launch, the
        streaming kernels one solve per frame; a kernel="coop" solver raises (unsupported
        configuration).  Stream-ordered, asynchronous.
        target_rot (device [T, B, 3, 3] float32, row-major rotations): pose targets
        (ikpso_solve_track_pose).  Every fitness then carries eff_w[tip] * orientation_weight *
        |R_eff - target_rot|_F^2, R_eff the world rotation of the effector NODE's frame (for a DH arm's
        tool frame pass DHArm.node_target(R_tool)); the stop tests and the returned fitness include it,
        the residual stays positional.  With weight 0 the answers equal the call without target_rot,
        bit for bit.  Only a FAST solver of a masked serial chain that folds, on the resident
        family, has the term; every other solver raises (unsupported configuration).  With
        target_rot=None this is ikpso_solve_track as before.
        aim_dir (device [T, B, 3] float32, world unit directions, used as given): aim targets
        (ikpso_solve_track_aim), for tasks that fix a tool axis and leave the roll about it free.  Every
        fitness then carries eff_w[tip] * aim_weight * |R_eff aim_axis - aim_dir|^2 instead, aim_axis
        (3 host values, normalised by the library) in the effector NODE's frame (for an axis of a DH
        arm's tool frame pass DHArm.node_axis(a_tool)).  The same solvers are served, weight 0 is
        again the call without the term bit for bit, and passing both target_rot and aim_dir raises
        ValueError.
        effector_rot (device [T, B, E, 3, 3] float32, row-major rotations, effectors in node order as in
        targets) with effector_rot_weight (a scalar or E host values, each finite and >= 0): orientation
        targets per effector (ikpso_solve_track_frames), for unmasked Euler chains and trees.  Every
        fitness then carries, added last, sum_e eff_w[e] * effector_rot_weight[e] * |R_e -
        effector_rot[e]|_F^2, R_e the world rotation of effector e's node frame; an effector of weight 0
        stays position-only.  Served is a FAST solver without axis mask or colliders on the resident
        family; every other solver raises (unsupported configuration).  With every weight 0 (or
        effector_rot_weight=None) the answers equal the call without the term, bit for bit.  Not
        combined with target_rot or aim_dir (ValueError)."""
        form = self._term_form(target_rot, orientation_weight, aim_dir, aim_axis, aim_weight, effector_rot,
                               effector_rot_weight)
        if targets is None or targets.dim() != 4:
            raise ValueError(f"targets must be [T, B, {self.effectors}, 3]")
        T, B = int(targets.shape[0]), int(targets.shape[1])
        it = self.pso.iterations if iterations is None else int(iterations)
        stop = -1.0 if stop_fitness is None else float(stop_fitness)
        if tuple(targets.shape) != (T, B, self.effectors, 3):
            raise ValueError(f"targets must be [{T}, {B}, {self.effectors}, 3]")
        if start_pose is not None and tuple(start_pose.shape) != (B, self.dof):
            raise ValueError(f"start_pose must be [{B}, {self.dof}]")
        outs = self._outputs((T, B), residual, self._device())
        self._solve_form(form, targets, start_pose, B, T, it, stop, outs, stream)
        return outs

    def sync(self) -> None:
        """ikpso_solver_sync: settle the last solve (see solve(sync=...))."""
        _abi.check(self._lib.ikpso_solver_sync(self._h), "ikpso_solver_sync")

    @property
    def fallbacks(self) -> int:
        """Cooperative solves of this solver that were re-run on the streaming kernels."""
        return int(self._lib.ikpso_solver_fallbacks(self._h))

    def generator_states(self, first_swarm: int = 0, count: Optional[int] = None, stream=None) -> np.ndarray:
        """The solver-owned generator states of local swarms [first_swarm, first_swarm + count):
        int32 words [count * P, 12] (curandState layout, swarm-major), after settling a
        pending solve (ikpso_solver_generator_states)."""
        n = (self.capacity - int(first_swarm)) if count is None else int(count)
        out = np.zeros((n * self.P, RNG_WORDS), dtype=np.int32)
        _abi.check(self._lib.ikpso_solver_generator_states(self._h, int(first_swarm), n, out.ctypes.data,
                                                           _stream_handle(stream)), "ikpso_solver_generator_states")
        return out

    def evaluate(self, angles, targets=None, rest=None, stream=None):
        """Device FK + fitness for angle vectors [n, D]: (fitness [n], node positions [n, J, 3])."""
        torch = _torch()
        n = int(angles.shape[0])
        if tuple(angles.shape) != (n, self.dof):
            raise ValueError(f"angles must be [n, {self.dof}]")
        for t, name in ((angles, "angles"), (targets, "targets"), (rest, "rest")):
            self._check_tensor(t, name, angles.device)
        fit = torch.empty((n,), dtype=torch.float32, device=angles.device)
        pos = torch.empty((n, self.chain.shape[0] - 1, 3), dtype=torch.float32, device=angles.device)
        _abi.check(self._lib.ikpso_solver_evaluate(self._h, _dev_ptr(angles), _dev_ptr(targets), _dev_ptr(rest), n,
                                                   _dev_ptr(fit), _dev_ptr(pos), _stream_handle(stream)),
                   "ikpso_solver_evaluate")
        return fit, pos

    def _evaluate_inputs(self, angles, targets=None, rest=None, effector_rot=None, effector_rot_weight=None):
        """The input checks of evaluate_frames(), gradient() and (angles alone) jacobian(): the shapes, the host
        weights, then the device layout.  Returns (n, the weights as _host_weights gives them)."""
        n, E = int(angles.shape[0]), self.effectors
        if tuple(angles.shape) != (n, self.dof):
            raise ValueError(f"angles must be [n, {self.dof}]")
        if targets is not None and tuple(targets.shape) != (n, E, 3):
            raise ValueError(f"targets must be [{n}, {E}, 3]")
        if rest is not None and tuple(rest.shape) != (n, self.dof):
            raise ValueError(f"rest must be [{n}, {self.dof}]")
        if effector_rot is not None and tuple(effector_rot.shape) != (n, E, 3, 3):
            raise ValueError(f"effector_rot must be [{n}, {E}, 3, 3]")
        host_w = self._host_weights(effector_rot_weight)
        for t, name in ((angles, "angles"), (targets, "targets"), (rest, "rest"), (effector_rot, "effector_rot")):
            self._check_tensor(t, name, angles.device)
        return n, host_w

    def evaluate_frames(self, angles, targets=None, rest=None, effector_rot=None, effector_rot_weight=None,
                        stream=None):
        """evaluate() with the node rotations and the orientation objective (ikpso_solver_evaluate_frames):
        (fitness [n], node positions [n, J, 3], node rotations [n, J, 3, 3], rot_error [n, E] or None).
        angles [n, D], targets [n, E, 3] or None and rest [n, D] or None are evaluate()'s.  effector_rot
        (device [n, E, 3, 3] float32, row-major, effectors in node order as in targets) gives rot_error, the
        unweighted |R_e - effector_rot[e]|_F^2 per effector (rotation_angle() turns it into the geodesic
        angle); without it rot_error is None.  effector_rot_weight (a scalar or E host values, each finite
        and >= 0; None: all 0) adds sum_e eff_w[e] * effector_rot_weight[e] * rot_error[e] to the fitness,
        last: the fitness solve_track(effector_rot=...) minimises, and with E = 1 the one
        solve_track(target_rot=..., orientation_weight=...) does.  Every solver evaluate() serves is served."""
        torch = _torch()
        E, J = self.effectors, self.chain.shape[0] - 1
        n, host_w = self._evaluate_inputs(angles, targets, rest, effector_rot, effector_rot_weight)
        fit = torch.empty((n,), dtype=torch.float32, device=angles.device)
        pos = torch.empty((n, J, 3), dtype=torch.float32, device=angles.device)
        rot = torch.empty((n, J, 3, 3), dtype=torch.float32, device=angles.device)
        err = None if effector_rot is None else torch.empty((n, E), dtype=torch.float32, device=angles.device)
        _abi.check(self._lib.ikpso_solver_evaluate_frames(self._h, _dev_ptr(angles), _dev_ptr(targets), _dev_ptr(rest),
                                                          _dev_ptr(effector_rot), host_w, n, _dev_ptr(fit),
                                                          _dev_ptr(pos), _dev_ptr(rot), _dev_ptr(err),
                                                          _stream_handle(stream)),
                   "ikpso_solver_evaluate_frames")
        return fit, pos, rot, err

    def jacobian(self, angles, stream=None):
        """The geometric Jacobian of every effector at given angle vectors (ikpso_solver_evaluate_jacobian):
        (jac [n, E, 6, D], node positions [n, J, 3]).  angles [n, D] is evaluate()'s.  jac[i, e] has rows 0..2
        d(position of effector e)/d(angle) and rows 3..5 the angular part, both in world coordinates, one
        column per free dimension in the solver's order (node order, then axis order); effectors in node
        order as in targets; a dimension off the effector's path to the root has a column of zeros.
        manipulability() takes the result.  Every solver evaluate() serves is served."""
        torch = _torch()
        E, J = self.effectors, self.chain.shape[0] - 1
        n, _ = self._evaluate_inputs(angles)
        jac = torch.empty((n, E, 6, self.dof), dtype=torch.float32, device=angles.device)
        pos = torch.empty((n, J, 3), dtype=torch.float32, device=angles.device)
        _abi.check(self._lib.ikpso_solver_evaluate_jacobian(self._h, _dev_ptr(angles), n, _dev_ptr(pos), _dev_ptr(jac),
                                                            _stream_handle(stream)),
                   "ikpso_solver_evaluate_jacobian")
        return jac, pos

    def contacts(self, angles, positions=False, stream=None):
        """Which node hits which collider at given angle vectors (ikpso_solver_evaluate_contacts): an int32
        tensor [n, C], C the colliders the solver was given (its own order, those left out as out of reach
        included: all-zero columns); with positions=True, (contacts, node positions [n, J, 3]).  angles
        [n, D] is evaluate()'s.  Bit k - 1 of contacts[i, c] is set when node k's node box or link box is
        decided to intersect collider c -- the decision behind evaluate()'s FLT_MAX: (contacts != 0).any(1)
        is exactly evaluate(...)[0] == FLT_MAX.  contact_nodes() and contact_pairs() decode the words.  Every
        solver evaluate() serves is served."""
        torch = _torch()
        J, C = self.chain.shape[0] - 1, self.colliders_given
        n, _ = self._evaluate_inputs(angles)
        out = torch.empty((n, C), dtype=torch.int32, device=angles.device)
        pos = torch.empty((n, J, 3), dtype=torch.float32, device=angles.device) if positions else None
        _abi.check(self._lib.ikpso_solver_evaluate_contacts(self._h, _dev_ptr(angles), n, _dev_ptr(out) if C else None,
                                                            _dev_ptr(pos), _stream_handle(stream)),
                   "ikpso_solver_evaluate_contacts")
        return (out, pos) if positions else out

    def gradient(self, angles, targets=None, rest=None, effector_rot=None, effector_rot_weight=None, stream=None):
        """The fitness evaluate_frames() reports and its gradient with respect to the angles
        (ikpso_solver_evaluate_gradient): (fitness [n], gradient [n, D]).  The arguments are evaluate_frames()'.
        gradient[i, d] is d fitness[i] / d angles[i, d] over every smooth term of the objective -- effector
        positions, the distance term, the angle term, the soft-limit penalty and the rotation term -- one
        column per free dimension in the solver's order.  A pose that collides has fitness FLT_MAX and the
        gradient of the smooth terms all the same.  Every solver evaluate() serves is served."""
        torch = _torch()
        n, host_w = self._evaluate_inputs(angles, targets, rest, effector_rot, effector_rot_weight)
        fit = torch.empty((n,), dtype=torch.float32, device=angles.device)
        grad = torch.empty((n, self.dof), dtype=torch.float32, device=angles.device)
        _abi.check(self._lib.ikpso_solver_evaluate_gradient(self._h, _dev_ptr(angles), _dev_ptr(targets), _dev_ptr(rest),
                                                            _dev_ptr(effector_rot), host_w, n, _dev_ptr(fit),
                                                            _dev_ptr(grad), _stream_handle(stream)),
                   "ikpso_solver_evaluate_gradient")
        return fit, grad

    def fitness(self, angles, targets=None, rest=None, effector_rot=None, effector_rot_weight=None, stream=None):
        """gradient()'s fitness [n] as a tensor on the autograd graph of `angles`: one
        ikpso_solver_evaluate_gradient call in the forward pass, whose gradient the backward pass scales by
        the incoming grad_output row by row.  Once differentiable, and with respect to `angles` alone (the
        other inputs get no gradient).  The device layout rules are gradient()'s."""
        torch = _torch()
        solver = self

        class _Fitness(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x):
                fit, grad = solver.gradient(x.detach(), targets, rest, effector_rot, effector_rot_weight, stream)
                ctx.save_for_backward(grad)
                return fit

            @staticmethod
            @torch.autograd.function.once_differentiable
            def backward(ctx, grad_output):
                (grad,) = ctx.saved_tensors
                return grad_output[:, None] * grad

        return _Fitness.apply(angles)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.ikpso_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
