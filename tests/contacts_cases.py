"""Chains, colliders and checkers of the contacts tests (tests/test_contacts.py on the CPU,
tests/test_gpu_contacts.py on the GPU).  Test infrastructure, imported like tests/topologies.py; nothing
here touches a GPU.

  * case(name): (chain, boxes, axis mask or None) of one test chain; NAMES lists them;
  * poses(name): the 600 angle vectors of a case over its free axes, uniform in [0, 2 pi);
  * oracle_bits(oracle, name): [600, C] words from the oracle's orc_node_collides, one call per (pose, node,
    collider) -- the reference's decision, what REFERENCE arithmetic must give bit for bit;
  * sat_gaps(name): the float64 separating-axis checker of the FAST decisions.

The boxes of every case are placed so that both outcomes occur (0.05 < share of colliding poses < 0.95);
tests/test_contacts.py holds the placement to that on the CPU.
"""
import functools

import numpy as np

import ikpso
import topologies as topo

N_POSES = 600  # two full 256-lane workgroups and a tail
GIZMO = 0.2
# the stated figures of tests/test_gpu_collide.py: GJK counts boxes within 3.5e-4 of touching, FAST frames
# differ from the reference's by up to 2e-5
GJK_BAND = 3.5e-4 + 2e-5
NAMES = ("scene4", "scene6", "generic1", "generic5", "serial20", "masked", "masked_wide")
# the chains whose FAST contacts are decided by separating axes; the others run GJK in FAST too
SAT_ROUTE = ("scene4", "scene6", "serial20", "masked")


def random_boxes(rng, n, centre, spread, lo=0.2, hi=1.2):
    """n boxes with random unit quaternions, edges in [lo, hi], centres within `spread` of `centre`."""
    c = np.zeros(n, dtype=ikpso.COLLIDER_DTYPE)
    for i in range(n):
        q = rng.normal(size=4)
        c[i]["x"], c[i]["y"], c[i]["z"] = rng.uniform(lo, hi, 3)
        c[i]["pos"] = np.asarray(centre) + rng.uniform(-spread, spread, 3)
        c[i]["quat"] = q / np.linalg.norm(q)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    scene = ikpso.reference_scene(reset=True).origin.to_cuda()
    if name == "scene4":
        return scene, ikpso.init_colliders(4), None
    if name == "scene6":  # beyond kNearUnroll = 4: the near test's loop runs
        return scene, random_boxes(np.random.default_rng(21), 6, (0, 0, 0), 2.5), None
    if name == "generic1":
        c = topo.random_tree(1, 0)
        return c, random_boxes(np.random.default_rng(31), 1, c["position"][0], 0.45, 0.5, 0.9), None
    if name == "generic5":  # no TopoSerialTip<5>, not the reference tree: TopoGeneric<5>
        c = topo.random_tree(5, 0)
        return c, random_boxes(np.random.default_rng(41), 3, c["position"][0], 1.5, 0.4, 1.0), None
    if name == "serial20":
        c = topo.serial(20)
        return c, random_boxes(np.random.default_rng(51), 5, c["position"][0], 1.6, 0.3, 0.9), None
    if name in ("masked", "masked_wide"):
        mask = np.full(len(scene), 7, dtype=np.uint8)
        mask[3] = 0b011  # node 3's z axis locked
        c = scene.copy()
        if name == "masked_wide":  # a clamp bound beyond the hardware sin/cos range: the masked collider builds
            c["max_rotation"][2][1] = 200.0
        return c, ikpso.init_colliders(4), mask
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def poses(name):
    chain, _, mask = case(name)
    d = len(topo.free_axes(chain, mask))
    rng = np.random.default_rng([7, NAMES.index(name)])
    return rng.uniform(0, 2 * np.pi, (N_POSES, d)).astype(np.float32)


def full_angles(name):
    chain, _, mask = case(name)
    return topo.expand(chain, poses(name), mask)


@functools.lru_cache(maxsize=None)
def _oracle_bits(name):
    import oracle

    lib = oracle.load()
    chain, boxes, _ = case(name)
    J, C = len(chain) - 1, len(boxes)
    bx = np.ascontiguousarray(boxes).view(oracle.BOX_DTYPE)
    out = np.zeros((N_POSES, C), dtype=np.uint32)
    for i, a in enumerate(full_angles(name)):
        M = np.ascontiguousarray(oracle.chain_matrices(chain, a))
        for k in range(1, J + 1):
            mk, mp = M[k].ctypes.data, M[int(chain["parent_index"][k])].ctypes.data
            for c in range(C):
                if lib.orc_node_collides(mk, mp, float(chain["length"][k]), bx[c:c + 1].ctypes.data, 1):
                    out[i, c] |= np.uint32(1 << (k - 1))
    out.setflags(write=False)
    return out


def oracle_bits(oracle, name):
    """[600, C] uint32, read-only, computed once per process."""
    return _oracle_bits(name)


# ------------------------------------------------------------------ the float64 separating-axis checker
def frames64(chain, full):
    """(R [n, J + 1, 3, 3], p [n, J + 1, 3]) of full Euler vectors [n, 3 J], from the definition, float64."""
    ang = np.asarray(full, dtype=np.float64).reshape(len(full), -1, 3)
    n, J = ang.shape[0], len(chain) - 1
    o = np.asarray(chain["rotation"][0], dtype=np.float64)
    R = np.zeros((n, J + 1, 3, 3))
    p = np.zeros((n, J + 1, 3))
    R[:, 0] = topo._rot(0, o[0:1]) @ topo._rot(1, o[1:2]) @ topo._rot(2, o[2:3])
    p[:, 0] = np.asarray(chain["position"][0], dtype=np.float64)
    for k in range(1, J + 1):
        par = int(chain["parent_index"][k])
        R[:, k] = R[:, par] @ topo._rot(0, ang[:, k - 1, 0]) @ topo._rot(1, ang[:, k - 1, 1]) @ topo._rot(2, ang[:, k - 1, 2])
        p[:, k] = p[:, par] + float(chain["length"][k]) * R[:, k, :, 0]
    return R, p


def quat_matrix(q):
    """The linear map v -> quatRotVec(v, q) of a collider's quaternion (x, y, z, w), float64: a rotation for a
    unit quaternion."""
    x, y, z, w = (float(v) for v in q)
    r = np.array([x, y, z])
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return (1 - 2 * r @ r) * np.eye(3) + 2 * np.outer(r, r) + 2 * w * K


def sat_gap(ca, A, ea, cb, B, eb):
    """The signed gap of oriented boxes by Gottschalk's 15 axes, vectorised over the leading dimension: centres
    c [n, 3], axes as matrix columns [n, 3, 3], half extents e [n, 3] (b: one box, broadcast).  The largest
    separation over the axes, each of unit length; an edge-pair axis with a cross product shorter than 1e-9 is
    skipped.  > 0: separated by that much along the best axis; <= 0: overlapping."""
    t = cb - ca
    gap = np.full(len(ca), -np.inf)

    def along(L):  # L [n, 3] unit
        ra = np.sum(ea * np.abs(np.einsum("nij,ni->nj", A, L)), axis=1)
        rb = np.sum(eb * np.abs(np.einsum("nij,ni->nj", B, L)), axis=1)
        return np.abs(np.sum(t * L, axis=1)) - ra - rb

    for i in range(3):
        gap = np.maximum(gap, along(A[:, :, i]))
        gap = np.maximum(gap, along(B[:, :, i]))
    for i in range(3):
        for j in range(3):
            L = np.cross(A[:, :, i], B[:, :, j])
            nrm = np.linalg.norm(L, axis=1)
            ok = nrm >= 1e-9
            g = along(L / np.where(ok, nrm, 1.0)[:, None])
            gap = np.where(ok, np.maximum(gap, g), gap)
    return gap


@functools.lru_cache(maxsize=None)
def sat_gaps(name):
    """(gap_node, gap_link, near) [600, J, C]: the float64 gaps of every node box and link box against every
    collider, and which pairs pass the sphere prefilter (the bounding spheres of the collider and of either
    box intersect)."""
    chain, boxes, _ = case(name)
    R, p = frames64(chain, full_angles(name))
    n, J, C = len(R), len(chain) - 1, len(boxes)
    gn, gl, near = np.zeros((n, J, C)), np.zeros((n, J, C)), np.zeros((n, J, C), dtype=bool)
    for c in range(C):
        b = boxes[c]
        M = quat_matrix(b["quat"])
        s = np.linalg.norm(M, axis=0)
        B = np.broadcast_to(M / s, (n, 3, 3))
        eb = np.broadcast_to(0.5 * np.abs([b["x"], b["y"], b["z"]]).astype(np.float64) * s, (n, 3))
        cb = np.broadcast_to(np.asarray(b["pos"], dtype=np.float64), (n, 3))
        for k in range(1, J + 1):
            par = int(chain["parent_index"][k])
            ln = abs(float(chain["length"][k]))
            en = np.broadcast_to(np.full(3, GIZMO / 2), (n, 3))
            el = np.broadcast_to(np.array([ln / 2, GIZMO / 8, GIZMO / 8]), (n, 3))
            mid = 0.5 * (p[:, k] + p[:, par])
            gn[:, k - 1, c] = sat_gap(p[:, k], R[:, k], en, cb, B, eb)
            gl[:, k - 1, c] = sat_gap(mid, R[:, k], el, cb, B, eb)
            rb = np.linalg.norm(eb[0])
            near[:, k - 1, c] = (np.linalg.norm(p[:, k] - cb, axis=1) <= np.linalg.norm(en[0]) + rb) | \
                                (np.linalg.norm(mid - cb, axis=1) <= np.linalg.norm(el[0]) + rb)
    return gn, gl, near


def expected_bits(name, band):
    """(hit, decided) [600, J, C] bool: what the float64 checker says of a pair's bit (the OR of its two boxes)
    wherever no gap within `band` of zero could turn it: hit when a box overlaps by more than the band, clear
    when both are apart by more than it."""
    gn, gl, _ = sat_gaps(name)
    hit = (gn < -band) | (gl < -band)
    clear = (gn > band) & (gl > band)
    return hit, hit | clear


def unpack(words, J):
    """[n, C] words -> [n, J, C] bool."""
    w = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    return ((w[:, None, :] >> np.arange(J)[None, :, None]) & 1).astype(bool)
