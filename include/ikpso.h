/*
 * ikpso.h -- C ABI of the MI355X-native PSO inverse-kinematics solver.
 *
 * This is the drop-in boundary for the reference's solver hot path
 * (MadDevX/Inverse-Kinematics-PSO-Research, src/ = InverseKinematicsResearch/
 * InverseKinematicsResearch/).  Plain C types, plain pointers and sizes; no
 * torch or C++ types.  Every entry point returns an ikpso_status (0 = success,
 * mirroring cudaSuccess/hipSuccess: the reference's caller aborts its frame
 * loop on any non-zero value, src/Main.cpp:225-226).
 *
 * Memory: "device" pointers are HIP device allocations (hipMalloc) or managed
 * allocations (hipMallocManaged); "any" pointers may be host, managed or device
 * memory (copied with hipMemcpyDefault).  Stream: a hipStream_t passed as
 * void*; NULL = the legacy default stream.  Calls are stream-ordered; the
 * reference-compatible entry points additionally synchronise before returning,
 * as the reference does (src/kernel.cu:317-322).
 */
#ifndef IKPSO_H
#define IKPSO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IKPSO_ABI_VERSION 5

typedef int ikpso_status;
enum {
    IKPSO_OK = 0,
    IKPSO_ERR_INVALID_ARG = 1,   /* bad size, null pointer, bad node table */
    IKPSO_ERR_UNSUPPORTED = 2,   /* no compiled kernel for this chain / swarm size / kernel family */
    IKPSO_ERR_HIP = 3,           /* a HIP runtime call failed; see ikpso_last_hip_error() */
    IKPSO_ERR_NO_MEMORY = 4
};

/* Node types, same values as the reference's NodeType (src/Particle.h:10-15). */
enum { IKPSO_NODE_ORIGIN = 0, IKPSO_NODE_EFFECTOR = 1, IKPSO_NODE = 2 };

/* One node of the kinematic tree; byte-identical to the reference's NodeCUDA
 * (src/Particle.h:24-39, 88 bytes).  Node 0 is the origin; nodes 1..J are
 * 3-axis Euler-XYZ joints followed by a link of `length` along local +X
 * (src/kernel.cu:52-56); parent_index < own index (DFS order, src/Node.h:232-267). */
typedef struct ikpso_node {
    int32_t node_type;
    int32_t parent_index;
    float effector_weight;
    float position[3];        /* origin only */
    float rotation[3];        /* current pose = warm start + angle-term reference */
    float max_rotation[3];    /* clamp bounds, per Euler axis */
    float min_rotation[3];
    float length;
    float target_position[3]; /* effectors only */
    float target_rotation[3]; /* unused by the fitness (as in the reference); orientation targets are
                                 an argument of ikpso_solve_track_pose and ikpso_solve_track_frames */
} ikpso_node;

/* XORWOW generator state with cuRAND's curandStateXORWOW layout (48 bytes),
 * so N * sizeof(curandState_t) allocations stay valid (src/Main.cpp:137). */
typedef struct ikpso_rng_state {
    uint32_t d;
    uint32_t v[5];
    int32_t boxmuller_flag;
    int32_t boxmuller_flag_double;
    float boxmuller_extra;
    uint32_t pad_;
    double boxmuller_extra_double;
} ikpso_rng_state;

/* PSOConfig (src/Particle.h:70-85): passed by value like the reference. */
typedef struct ikpso_pso_config {
    float inertia;
    float local;
    float global;
    int32_t iterations;
} ikpso_pso_config;

/* FitnessConfig (src/Particle.h:55-68). */
typedef struct ikpso_fitness_config {
    float angle_weight;
    float distance_weight;
    float error_threshold; /* never read, as in the reference */
} ikpso_fitness_config;

/* obj_t (src/BoxCollider.h:4-10): box edge lengths x, y, z (supportBox uses
 * +-x/2), centre, orientation quaternion (x, y, z, w). */
typedef struct ikpso_collider {
    float x, y, z;
    float pos[3];
    float pad_[2];
    float quat[4]; /* float4, 16-byte aligned in the reference */
} ikpso_collider;

/* Kernel family (ikpso_solver_desc.kernel; env IKPSO_KERNEL for ikpso_calculate_pso). */
enum {
    IKPSO_KERNEL_AUTO = 0,      /* resident when the swarm fits one workgroup, else cooperative, else streaming */
    IKPSO_KERNEL_RESIDENT = 1,  /* one workgroup per swarm, state on chip, one launch per batch */
    IKPSO_KERNEL_STREAMING = 2, /* state in HBM, one launch per iteration, any swarm size */
    IKPSO_KERNEL_COOP = 3       /* one swarm over G co-resident workgroups (G CUs), state on chip, one
                                   launch per batch; AUTO picks it for swarms above one workgroup when
                                   the chain has a specialised kernel and G <= CUs / 8 */
};

/* Arithmetic mode of the device kernels. */
enum {
    IKPSO_ARITH_FAST = 0,      /* closed-form 3x3 FK, FMA contraction (default); sin/cos on the
                                  transcendental unit when every clamp bound and rest angle of the
                                  chain lies within +-100 rad (the answers are clamped there), else a
                                  1-ulp polynomial.  A start pose (or the rest pose of the compat
                                  call) beyond +-100 rad inside such bounds is evaluated once, at
                                  initialisation, with the unit's larger error there (~1e-5 at 150 rad);
                                  every later evaluation is of clamped angles.  The resident and
                                  cooperative FAST kernels keep angles in revolutions (x / 2pi), so
                                  answers and dumped particles come back within 4 ulp of the radian
                                  values -- at 0 iterations the rest pose within 4 ulp, not bit for
                                  bit (REFERENCE returns it exactly) */
    IKPSO_ARITH_REFERENCE = 1  /* the reference's 4x4 operation order, no FMA contraction */
};

/* ---------------------------------------------------------------------------
 * Reference-compatible entry points (single swarm).
 * ------------------------------------------------------------------------- */

/* Replaces initGenerators (src/utility_kernels.cuh:33-47, declared at
 * src/Main.cpp:28): randoms[i] = curand_init(i, 0, 0).  randoms: device. */
ikpso_status ikpso_init_generators(ikpso_rng_state* randoms, int size, void* stream);

/* Generalised seeding: randoms[i] = curand_init(seed_base + i, 0, 0). */
ikpso_status ikpso_init_generators_seeded(ikpso_rng_state* randoms, int64_t count, uint64_t seed_base,
                                          void* stream);

/* Replaces calculatePSO (src/kernel.cu:279-327, declared at src/Main.cpp:29).
 *   particles [3][D][size] floats, device: SoA position / velocity / local best
 *             (src/kernel.cu:17-29); overwritten with the final swarm state.
 *   positions [4*J] floats, any: host-computed arm positions, read only when
 *             fit.distance_weight != 0, at slot (k-1)*4 for node k (src/kernel.cu:94-98);
 *             [4*(J+2)] read at slot (k+1)*4 with IKPSO_POSREF=node_slot (see IKPSO_FLAG_*).
 *   bests     [size] floats, device: final local-best fitness per particle.
 *   randoms   [size] states, device: consumed and advanced (persist across calls).
 *   chain     [node_count] nodes, any.  D = 3*(node_count-1).
 *   result    [D] floats, any: global-best joint angles (Coordinates).
 *   colliders [collider_count] obj_t, any: boxes of the collider term (src/kernel.cu:104-136):
 *             a particle whose node or link box intersects one (GJK) gets fitness FLT_MAX.
 * Synchronises `stream` before returning.  After the argument checks, an error the
 * caller's earlier HIP work left pending (unread by hipGetLastError) is returned
 * (IKPSO_ERR_HIP, ikpso_last_hip_error) and consumed up front, and nothing runs:
 * particles, bests, randoms and result are left untouched.  The reference returns
 * such an error too (its first cudaGetLastError check, src/kernel.cu:293-295), but
 * only after its init kernels have rewritten particles, bests and randoms.
 * ikpso_solver_create and ikpso_solve_batch take a pending error the same way
 * (a stale error from unrelated earlier work fails them; read it with
 * hipGetLastError first to avoid that). */
ikpso_status ikpso_calculate_pso(float* particles, const float* positions, float* bests,
                                 ikpso_rng_state* randoms, int size, const ikpso_node* chain, int node_count,
                                 ikpso_pso_config pso, ikpso_fitness_config fit, float* result,
                                 const ikpso_collider* colliders, int collider_count, void* stream);

/* ---------------------------------------------------------------------------
 * Batched API: B independent swarms (IK targets) per call, one launch.
 * ------------------------------------------------------------------------- */

typedef struct ikpso_solver ikpso_solver;

typedef struct ikpso_solver_desc {
    const ikpso_node* chain;  /* any; node table shared by every swarm */
    int32_t node_count;       /* J + 1 */
    int32_t particles;        /* P per swarm */
    ikpso_pso_config pso;
    ikpso_fitness_config fit;
    int32_t arith;            /* IKPSO_ARITH_* */
    int32_t kernel;           /* IKPSO_KERNEL_* */
    const float* positions;   /* any, [4*J] or NULL (distance term, as calculatePSO) */
    /* Optional soft joint-limit penalty (a new term; the reference only clamps):
     * fitness += limit_weight * sum_d max(0, x_d - soft_hi[d], soft_lo[d] - x_d)^2 */
    float limit_weight;
    float reserved1;
    const float* soft_lo;     /* any, [D] or NULL */
    const float* soft_hi;     /* any, [D] or NULL */
    /* Collider term, as calculatePSO's colliders/colliderCount (ABI >= 2). */
    const ikpso_collider* colliders; /* any, [collider_count] or NULL */
    int32_t collider_count;
    int32_t flags;            /* IKPSO_FLAG_* */
    /* Joint-axis mask (ABI >= 4; an extension -- the reference hard-wires three
     * Euler axes per node, src/kernel.cu:52-56,160-187): any, [node_count] or
     * NULL.  Bit c of axis_mask[k] set = Euler angle c of node k is a PSO
     * dimension; a clear bit locks that angle at the node's rotation[c] (no
     * draws, no update, no clamp; the angle term sees an exact zero).  Entry 0
     * (the origin) is ignored.  NULL = every axis free = the reference.  D, the
     * solver's dimension count, is then the number of free axes: start poses,
     * answers, soft limits and evaluate()'s angles carry those D values in node
     * order, axis order within a node.  FAST solves of a serial chain with a
     * tip effector and no distance/collider term run on the chain folded into
     * its free axes (one sincos per free angle; DH arms); see IKPSO_FLAG_NO_FOLD. */
    const uint8_t* axis_mask;
} ikpso_solver_desc;

/* ikpso_solver_desc.flags (env IKPSO_POSREF=node_slot for ikpso_calculate_pso). */
enum {
    /* Distance term with the reference's latent slot bug fixed (opt-in): the
     * reference reads node k's reference position from positions[(k-1)*4],
     * which FillPositions (src/Node.h:110-149) filled with node k-2's; with
     * this flag positions is [4*(J+2)] as FillPositions writes it and node k
     * reads slot k+1, its own.  Off: bit-compatible with the reference. */
    IKPSO_FLAG_POSREF_NODE_SLOT = 1,
    /* Solve a masked chain with the Euler kernels (locked axes skipped) even
     * where the folded form applies (ABI >= 4; comparisons and tests). */
    IKPSO_FLAG_NO_FOLD = 2
};

ikpso_status ikpso_solver_create(const ikpso_solver_desc* desc, ikpso_solver** out);
ikpso_status ikpso_solver_destroy(ikpso_solver* solver);

/* Allocate (or re-seed) the solver-owned generator states for `capacity`
 * swarms: state of local swarm b, particle i = curand_init(seed_base +
 * (first_swarm + b) * P + i, 0, 0).  first_swarm is the global index of local
 * swarm 0, so a batch sharded over ranks draws the same streams as one rank.
 * States persist across solve calls (like the reference's randoms buffer). */
ikpso_status ikpso_solver_seed(ikpso_solver* solver, int64_t capacity, uint64_t seed_base, int64_t first_swarm,
                               void* stream);

/* Solve `num_swarms` (<= capacity) swarms for `iterations` PSO iterations.
 *   targets    device, [B][E][3]: effector targets, effectors in node order.
 *   start_pose device, [B][D] or NULL (NULL: chain rotations).
 *   out_angles device [B][D]; out_fitness device [B]; out_residual device [B] or NULL
 *   (residual = sum over effectors of |p_e - t_e|, as checkDistance).
 * Stream-ordered; does not synchronise.  A solver handle owns one workspace:
 * calls on one handle must be ordered (one stream, or synchronised), not
 * concurrent.  The cooperative family needs its workgroups co-resident (one per
 * CU): the grid is checked against the occupancy query at launch, and if other
 * work on the device still keeps a group from assembling, its bounded wait
 * gives up (never a hang) and the swarms it had not finished get NaN angles,
 * fitness and residual -- until ikpso_solver_sync settles the solve. */
ikpso_status ikpso_solve_batch(ikpso_solver* solver, const float* targets, const float* start_pose,
                               int64_t num_swarms, int32_t iterations, float* out_angles, float* out_fitness,
                               float* out_residual, void* stream);

/* Solve to a fitness tolerance: solve_batch with a per-swarm early stop (added
 * after ABI 5; detect by symbol).  The arguments are solve_batch's, plus
 *   stop_fitness   threshold on the FITNESS, the quantity PSO minimises (the
 *                  weighted distance, angle and optional terms) -- not on the
 *                  residual.  Negative: never stop.  NaN: IKPSO_ERR_INVALID_ARG.
 *   out_iterations device, [B] or NULL: iterations each swarm ran.
 * Swarm b stops after the first iteration n >= 0 at which its global-best
 * fitness is <= stop_fitness (n = 0: the initial global best, before any PSO
 * iteration, already meets it); otherwise it runs max_iterations.  A stopped
 * swarm's outputs and generator states are those of solve_batch with
 * iterations = n, bit for bit: a particle has drawn D + 3 D n values, no more.
 * Stream-ordered; does not synchronise.  Runs the resident kernel (where a
 * stopped swarm's workgroup ends and its CU takes the next swarm) or the
 * streaming kernels (a stopped swarm's chunks idle through the remaining
 * launches).  The cooperative kernels have no stop: a solver that AUTO routed to
 * them runs the streaming kernels here, a resident solver never takes the
 * few-swarm cooperative route, and a solver created with IKPSO_KERNEL_COOP gets
 * IKPSO_ERR_UNSUPPORTED. */
ikpso_status ikpso_solve_batch_until(ikpso_solver* solver, const float* targets, const float* start_pose,
                                     int64_t num_swarms, int32_t max_iterations, float stop_fitness,
                                     float* out_angles, float* out_fitness, float* out_residual,
                                     int32_t* out_iterations, void* stream);

/* Follow a sequence of targets: `frames` solves of every swarm in one call, each
 * warm-started from the answer of the one before (added after ABI 5; detect by
 * symbol).  Layouts are time-major, so frame t of every buffer is what one
 * solve_batch_until call takes:
 *   targets        device, [T][B][E][3].
 *   start_pose     device, [B][D] or NULL: frame 0's only (NULL: chain rotations).
 *   out_angles     device, [T][B][D].
 *   out_fitness    device, [T][B].
 *   out_residual   device, [T][B] or NULL.
 *   out_iterations device, [T][B] or NULL.
 * Contract: frame t of swarm b is ikpso_solve_batch_until on targets[t] with
 * max_iterations and stop_fitness, its start_pose the caller's for t == 0 and
 * out_angles[t-1] for t > 0 -- bit for bit, in FAST as in REFERENCE arithmetic,
 * for the outputs, the iteration counts and the generator states left in the
 * solver after the last frame.  Every frame is a fresh swarm (positions and rest
 * pose at its start, velocities drawn, local bests at the positions); only the
 * generators carry on from frame to frame.  A negative stop_fitness never stops;
 * NaN is IKPSO_ERR_INVALID_ARG, even with nothing to solve.  frames == 0 or
 * num_swarms == 0 returns IKPSO_OK with no device work; frames > 0 needs targets
 * and out_angles.  Stream-ordered; does not synchronise.
 * The resident family runs the whole call in one launch: a swarm stays on its CU
 * and its generator states in registers for all frames.  A streaming solver, or
 * one that AUTO routed to the cooperative family, runs one streaming solve per
 * frame; a solver created with IKPSO_KERNEL_COOP gets IKPSO_ERR_UNSUPPORTED.  A
 * pending cooperative solve is settled first. */
ikpso_status ikpso_solve_track(ikpso_solver* solver, const float* targets, const float* start_pose,
                               int64_t num_swarms, int32_t frames, int32_t max_iterations, float stop_fitness,
                               float* out_angles, float* out_fitness, float* out_residual,
                               int32_t* out_iterations, void* stream);

/* Pose targets: ikpso_solve_track with a tip orientation term (added after ABI 5;
 * detect by symbol).  Every fitness of the call -- the local and global bests, the
 * per-frame stop test, out_fitness -- is ikpso_solve_track's plus, added last,
 *   effector_weight[tip] * orientation_weight * |R_eff - R_target|_F^2
 * where R_eff is the world rotation of the EFFECTOR NODE's frame as the Euler chain
 * defines it (the origin's Rx Ry Rz, then Rx Ry Rz of every node down to the
 * effector, locked axes at their rotation[]; the link translation does not turn the
 * frame) and R_target the caller's rotation.  The squared Frobenius distance is
 * 4 (1 - cos theta) for the geodesic angle theta between the two.  A DH arm's tool
 * frame differs from the node frame by a constant rotation (ikpso.dh.DHArm
 * .tool_rotation; node_target converts).
 *   target_rot          device, [T][B][9]: row-major 3x3 rotations, time-major like
 *                       targets; may be NULL when orientation_weight == 0.
 *   orientation_weight  >= 0.  With 0 every output, iteration count and generator
 *                       state equals ikpso_solve_track's, bit for bit (the term is
 *                       absent, and the call runs the track kernel without it; the
 *                       kernels with the term evaluate the position term by the
 *                       same expressions, whose FMA contraction may differ by an
 *                       ulp from kernel to kernel, as between any two FAST builds).
 * Every other argument, and the contract (a fresh swarm per frame warm-started from
 * the previous answer; the per-frame early stop on the whole fitness, this term
 * included; frames == 1 is the pose form of solve_batch_until, a negative
 * stop_fitness that of solve_batch), are ikpso_solve_track's.  out_residual stays
 * the positional checkDistance residual.  A particle draws D + 3 D n values, as
 * without the term.
 * IKPSO_ERR_INVALID_ARG: a NaN or negative orientation_weight, a NaN stop_fitness,
 * frames > 0 with a NULL targets or out_angles, orientation_weight > 0 with a NULL
 * target_rot.
 * IKPSO_ERR_UNSUPPORTED: only the folded chain's resident track kernels have the
 * term, and no kernel without it is ever run in their place.  So every solver but
 * a FAST one of a masked serial chain with a tip effector that folds (see
 * axis_mask), created on the resident family with a swarm that fits one
 * workgroup, is refused: REFERENCE arithmetic, IKPSO_FLAG_NO_FOLD, an unmasked
 * chain, a tree, a chain with a distance or collider term, a streaming or
 * cooperative solver (requested, or picked by AUTO for a swarm above one
 * workgroup).  The refusal comes before the frames == 0 / num_swarms == 0 return
 * (IKPSO_OK, no device work).
 * ikpso_solver_evaluate is unchanged: its fitness never includes this term. */
ikpso_status ikpso_solve_track_pose(ikpso_solver* solver, const float* targets, const float* target_rot,
                                    float orientation_weight, const float* start_pose, int64_t num_swarms,
                                    int32_t frames, int32_t max_iterations, float stop_fitness, float* out_angles,
                                    float* out_fitness, float* out_residual, int32_t* out_iterations,
                                    void* stream);

/* Aim targets: ikpso_solve_track with a tool-axis term, the roll about the axis left
 * free (added after ABI 5; detect by symbol).  Every fitness of the call -- the local
 * and global bests, the per-frame stop test, out_fitness -- is ikpso_solve_track's
 * plus, added last,
 *   effector_weight[tip] * aim_weight * |R_eff a - d|^2
 * where R_eff is the world rotation of the EFFECTOR NODE's frame exactly as
 * ikpso_solve_track_pose defines it, a the caller's axis in that node frame and d the
 * frame's world direction.  For unit vectors the value is 2 (1 - cos phi), phi the
 * angle between the tool axis and the direction; a rotation of the tool about a does
 * not change it, so the term takes 2 of the 3 orientation degrees of freedom.  For
 * an axis named in a DH arm's tool frame see ikpso.dh.DHArm.node_axis.
 *   aim_dir     device, [T][B][3], time-major like targets.  Used AS GIVEN: pass unit
 *               vectors; a non-unit d gives the expression above and nothing else.
 *               May be NULL when aim_weight == 0.
 *   aim_axis    HOST memory, 3 floats, read during the call; the same for every swarm
 *               and frame.  Finite, of norm >= 1e-6; the library normalises it (in
 *               fp64).  May be NULL when aim_weight == 0.
 *   aim_weight  >= 0.  With 0 the term is absent and the call runs the track kernel
 *               without it: every output, iteration count and generator state equals
 *               ikpso_solve_track's, bit for bit (as ikpso_solve_track_pose at
 *               weight 0).
 * Every other argument, and the contract (a fresh swarm per frame warm-started from
 * the previous answer; the per-frame early stop on the whole fitness, this term
 * included; frames == 1 is the aim form of solve_batch_until, a negative stop_fitness
 * never stops), are ikpso_solve_track's.  out_residual stays the positional
 * checkDistance residual.  A particle draws D + 3 D n values, as without the term.
 * IKPSO_ERR_INVALID_ARG: a NaN or negative aim_weight, a NaN stop_fitness, frames > 0
 * with a NULL targets or out_angles, aim_weight > 0 with a NULL aim_dir, or with a
 * NULL, non-finite or near-zero (norm < 1e-6) aim_axis.
 * IKPSO_ERR_UNSUPPORTED: exactly the solvers ikpso_solve_track_pose refuses (only a
 * FAST, folded, resident solver whose swarm fits one workgroup is served), before the
 * frames == 0 / num_swarms == 0 return (IKPSO_OK, no device work).
 * The aim and the orientation term are not combined: a call has one or the other.
 * ikpso_solver_evaluate is unchanged: its fitness never includes this term. */
ikpso_status ikpso_solve_track_aim(ikpso_solver* solver, const float* targets, const float* aim_dir,
                                   const float* aim_axis, float aim_weight, const float* start_pose,
                                   int64_t num_swarms, int32_t frames, int32_t max_iterations,
                                   float stop_fitness, float* out_angles, float* out_fitness,
                                   float* out_residual, int32_t* out_iterations, void* stream);

/* Orientation targets per effector for Euler chains and trees: ikpso_solve_track with a
 * rotation term for every effector (added after ABI 5; detect by symbol).  Every fitness
 * of the call -- the local and global bests, the per-frame stop test, out_fitness -- is
 * ikpso_solve_track's plus, accumulated over the effectors in node order and added last,
 *   sum_e effector_weight[k_e] * rot_weights[e] * |R_{k_e} - target_rot[e]|_F^2
 * where R_k is the world rotation of node k's frame as the Euler chain defines it (the
 * origin's Rx Ry Rz, then Rx Ry Rz of every node down the path to k; links do not turn
 * the frame: ikpso_solve_track_pose's definition) and k_e the node of effector e.
 *   target_rot   device, [T][B][E][9]: row-major 3x3 rotations, time-major like targets,
 *                effectors in node order exactly as targets indexes them; used as given.
 *                May be NULL when every weight is 0.
 *   rot_weights  HOST memory (as aim_axis is), E floats read during the call; the same
 *                weights for every swarm and frame.  Each finite and >= 0; a weight of 0
 *                leaves that effector position-only (fingertips).  NULL: all weights 0.
 * With all weights 0 (or NULL) the call runs the kernel ikpso_solve_track runs and equals
 * it bit for bit in outputs, iteration counts and generator states (the kernels with the
 * term evaluate the position term by the same expressions in the runtime-term build's
 * form, whose rounding may differ from a specialised build's, as between any two FAST
 * builds).
 * Everything else is ikpso_solve_track's contract: a fresh swarm per frame warm-started
 * from the previous answer; the per-frame stop on the whole fitness, this term included;
 * frames == 1 the form of solve_batch_until, a negative stop_fitness never stops; a
 * particle draws D + 3 D n values; out_residual stays the positional checkDistance
 * residual.  ikpso_solver_evaluate is unchanged: its fitness never includes this term.
 * IKPSO_ERR_INVALID_ARG: a NaN stop_fitness; a NaN, infinite or negative weight; some
 * weight > 0 with a NULL target_rot; frames > 0 with a NULL targets or out_angles.
 * IKPSO_ERR_UNSUPPORTED (before the frames == 0 / num_swarms == 0 return, which is
 * IKPSO_OK with no device work): served is a FAST solver of an unmasked Euler chain or
 * tree with no collider term that its kernels test -- any compiled topology: the
 * reference tree, the serial-tip widths, generic trees of 1..20 joints; the distance
 * term and the soft-limit penalty are allowed -- created on the resident family with a
 * swarm that fits one workgroup.  Refused: REFERENCE arithmetic; any axis mask, whether
 * it folds or not, IKPSO_FLAG_NO_FOLD included (folded arms have
 * ikpso_solve_track_pose); a chain whose collider term is live; a streaming or
 * cooperative solver, requested or picked by AUTO.  No kernel without the term is ever
 * run in the place of one with it. */
ikpso_status ikpso_solve_track_frames(ikpso_solver* solver, const float* targets, const float* target_rot,
                                      const float* rot_weights, const float* start_pose, int64_t num_swarms,
                                      int32_t frames, int32_t max_iterations, float stop_fitness,
                                      float* out_angles, float* out_fitness, float* out_residual,
                                      int32_t* out_iterations, void* stream);

/* Settle the last solve_batch (ABI >= 3).  After a cooperative-family solve:
 * wait for it and, if a group gave up (the GPU shared with other work), restore
 * the generator states from the snapshot taken before the launch and re-run the
 * batch on the streaming kernels, which need no co-residency, so the outputs are
 * always a complete solve.  Returns at once after the other families.  The
 * buffers passed to that solve_batch must still be valid.  solve_batch settles a
 * pending solve itself before it launches the next one. */
ikpso_status ikpso_solver_sync(ikpso_solver* solver);
/* Solves of this handle / of the process that took the streaming fallback. */
int64_t ikpso_solver_fallbacks(const ikpso_solver* solver);
int64_t ikpso_coop_fallbacks(void);

/* Evaluate the device FK + fitness for n angle vectors (no PSO):
 *   angles device [n][D]; targets device [n][E][3] or NULL (chain targets);
 *   rest device [n][D] or NULL (chain rotations); out_fitness device [n] or NULL;
 *   out_positions device [n][J][3] or NULL (world position of nodes 1..J).
 *   D = free dimensions (the axis mask); locked angles at the chain's rotation.
 *   Always the Euler form of the chain (a folded FAST solver's answers agree
 *   with it within the FAST tolerance). */
ikpso_status ikpso_solver_evaluate(ikpso_solver* solver, const float* angles, const float* targets,
                                   const float* rest, int64_t n, float* out_fitness, float* out_positions,
                                   void* stream);

/* ikpso_solver_evaluate with the node rotations, the rotation error per effector and the
 * rotation term of ikpso_solve_track_frames in the fitness (added after ABI 5; detect by
 * symbol): what the orientation entries optimise, reported for given angle vectors.
 *   angles, targets, rest, n, out_fitness, out_positions: exactly ikpso_solver_evaluate's
 *   (free dimensions under an axis mask, locked axes at the chain's rotation, NULL targets
 *   the chain's own, always the Euler form of the chain).
 *   out_rotations  device, [n][J][9] or NULL: the world rotation of the frames of nodes
 *                  1..J, row-major, as ikpso_solve_track_pose defines it (the origin's
 *                  Rx Ry Rz, then Rx Ry Rz of every node down the path; links do not
 *                  turn the frame).  FAST kernels on the hardware sin/cos add back
 *                  that unit's known amplitude bias (2 depth(k) * 3.23e-8 of node k's
 *                  rotation, as their link lengths carry it), so the matrices are
 *                  orthonormal to float32 rounding; out_rot_error and the term are
 *                  formed on the rotation returned here.
 *   target_rot     device, [n][E][9] or NULL: one row-major rotation per vector and
 *                  effector, effectors in node order as targets indexes them; used as
 *                  given.
 *   out_rot_error  device, [n][E] or NULL: the unweighted |R_{k_e} - target_rot[e]|_F^2
 *                  of every effector, the nine squared differences accumulated in
 *                  row-major order.  The value is 4 (1 - cos theta) for the geodesic
 *                  angle theta, with no weight in the way.  Needs target_rot.
 *   rot_weights    HOST memory (as in ikpso_solve_track_frames), E floats read during
 *                  the call, each finite and >= 0; NULL: all 0.
 * out_fitness is ikpso_solver_evaluate's fitness plus, accumulated over the effectors in
 * node order and added last,
 *   sum_e effector_weight[k_e] * rot_weights[e] * |R_{k_e} - target_rot[e]|_F^2
 * -- ikpso_solve_track_frames' expression, and for a folded arm (E = 1) also
 * ikpso_solve_track_pose's with orientation_weight = rot_weights[0] (the folded kernels
 * compute it in their own form: agreement is within the FAST tolerance, as for
 * ikpso_solver_evaluate).  A weight of 0 contributes nothing, and that effector's target
 * is never read into the sum.  A fitness the collider term set to FLT_MAX stays FLT_MAX.
 * With every weight 0 (or NULL) out_fitness and out_positions are ikpso_solver_evaluate's:
 * the same expressions in another kernel, so in REFERENCE arithmetic, where every
 * rounding is pinned, the same values; in FAST they may differ by the rounding any two
 * FAST builds differ by (FMA contraction is the compiler's, kernel by kernel).
 * Served is every solver ikpso_solver_evaluate serves -- FAST and REFERENCE, masked
 * chains, folded DH arms (through their Euler chain), trees, chains with colliders, every
 * compiled topology -- routed as evaluate routes it (a chain whose solve runs the masked
 * collider arithmetic is evaluated by it).  Nothing evaluate accepts is refused.
 * IKPSO_ERR_INVALID_ARG: what ikpso_solver_evaluate rejects; a NaN, infinite or negative
 * weight; some weight > 0 with a NULL target_rot; out_rot_error with a NULL target_rot.
 * n == 0 is IKPSO_OK with no device work.  Stream-ordered: the call does not
 * synchronise (the weights are read during the call), and like ikpso_solver_evaluate it
 * neither waits for nor settles a pending solve. */
ikpso_status ikpso_solver_evaluate_frames(ikpso_solver* solver, const float* angles, const float* targets,
                                          const float* rest, const float* target_rot, const float* rot_weights,
                                          int64_t n, float* out_fitness, float* out_positions,
                                          float* out_rotations, float* out_rot_error, void* stream);

/* The geometric Jacobian of every effector at given angle vectors, on the device (added
 * after ABI 5; detect by symbol): how the positions and rotations the evaluate entries
 * report change with the joint angles -- for a Gauss-Newton polish of an answer, velocity
 * IK between the frames of a track, manipulability and singularity checks.
 *   angles         exactly ikpso_solver_evaluate's: device, [n][D], the free dimensions
 *                  under an axis mask, locked axes at the chain's rotation, always the
 *                  Euler form of the chain.
 *   out_positions  device, [n][J][3] or NULL: ikpso_solver_evaluate's output, with the
 *                  caveat ikpso_solver_evaluate_frames states (in REFERENCE arithmetic
 *                  the same values; in FAST the rounding any two FAST builds differ by).
 *   out_jacobian   device, [n][E][6][D], required when n > 0.  Effectors in node order,
 *                  as targets indexes them; rows 0..2 the linear part, rows 3..5 the
 *                  angular part, both in world coordinates; columns the D free
 *                  dimensions in the solver's own order (node order, then axis order
 *                  within a node).
 * No targets, rest pose or weights: the Jacobian depends on none of them.
 * Definition, with the frames as ikpso_solve_track_pose defines them: node k's frame is
 * frame(parent(k)) Rx(x_k) Ry(y_k) Rz(z_k) T(length_k, 0, 0), frame(0) the origin's
 * position and fixed Rx Ry Rz; R_k is its rotation, p_k its position (p_0 the origin's).
 * For effector e at node m and free dimension d, the angle c of node k:
 *   k is m or an ancestor of m: the column is (a x (p_m - p_parent(k)), a), a the world
 *     axis of that angle,
 *       c = 0 (x): a = R_parent(k) e_x
 *       c = 1 (y): a = R_parent(k) Rx(x_k) e_y
 *       c = 2 (z): a = R_k e_z
 *     The angular part means dR_m / d theta_d = [a]x R_m.
 *   otherwise: all six entries are exactly +0.0f (the other wrists of the 7-node scene,
 *     the other fingers of a tree).
 * A DH arm is evaluated through its masked Euler chain, as ikpso_solver_evaluate does: its
 * D columns are the arm's joints, and the constant tool rotation between the effector
 * node's frame and the DH tool frame does not change the world angular velocity, so the
 * rows need no conversion.
 * FAST kernels on the hardware sin/cos take the axes from the rotation
 * ikpso_solver_evaluate_frames returns (that unit's known amplitude bias added back), so
 * |a| = 1 to float32 rounding; the positions are untouched, as in that entry.
 * Served is every solver ikpso_solver_evaluate serves -- FAST and REFERENCE, masked
 * chains, folded DH arms, trees, chains with colliders, every compiled topology -- routed
 * as evaluate routes it.  A collider changes nothing in the output; only the build's
 * arithmetic follows it.  Nothing evaluate accepts is refused.
 * IKPSO_ERR_INVALID_ARG: a NULL solver; n < 0; n > 0 with a NULL angles or a NULL
 * out_jacobian.  n == 0 is IKPSO_OK with no device work.  Stream-ordered: the call does
 * not synchronise, and like ikpso_solver_evaluate it neither waits for nor settles a
 * pending solve. */
ikpso_status ikpso_solver_evaluate_jacobian(ikpso_solver* solver, const float* angles, int64_t n,
                                            float* out_positions, float* out_jacobian, void* stream);

/* The fitness ikpso_solver_evaluate_frames reports and its gradient with respect to the joint
 * angles, on the device (added after ABI 5; detect by symbol): what a first-order or
 * quasi-Newton optimiser (L-BFGS-B with the joint bounds, projected gradient descent) needs to
 * polish a batch of PSO answers against the solver's own objective -- every term of it, the
 * distance term, the angle term and the soft-limit penalty included, which the effector
 * Jacobians alone do not cover.
 *   angles, targets, rest, target_rot, rot_weights (host memory, E floats), n
 *                  exactly ikpso_solver_evaluate_frames': the free dimensions under an axis
 *                  mask, locked axes at the chain's rotation, NULL targets the chain's own,
 *                  always the Euler form of the chain.
 *   out_fitness    device, [n] or NULL: the fitness ikpso_solver_evaluate_frames reports for
 *                  the same arguments, a collider's FLT_MAX included.
 *   out_gradient   device, [n][D], required when n > 0: column d is the derivative of that
 *                  fitness with respect to free dimension d, in the solver's own order (node
 *                  order, then axis order within a node).
 * Definition, with the frames R_k, p_k and the world axes a of
 * ikpso_solver_evaluate_jacobian.  For free dimension d, the angle c of node k, with
 * q = p_parent(k) the angle's pivot and S(k) node k and its descendants, the gradient is the
 * sum of
 *   effector positions   sum over the effectors m in S(k) of
 *                          2 eff_w[m] (p_m - t_m) . (a x (p_m - q))
 *   distance term        (distance_weight != 0 only) sum over every node m in S(k) of
 *                          2 dw (p_m - ref_m) . (a x (p_m - q)),
 *                        dw = distance_weight / J and ref_m the slot of the positions array
 *                        the fitness reads (IKPSO_FLAG_POSREF_NODE_SLOT or the reference's);
 *                        the constant (1 - ref_w)^2 of that term contributes nothing
 *   angle term           2 aw (x_d - rest_d), aw = angle_weight / J
 *   soft-limit penalty   2 limit_weight (x_d - soft_hi[d]) above the soft bound,
 *                        -2 limit_weight (soft_lo[d] - x_d) below it, 0 between and at the
 *                        bounds: the penalty is C1, so the gradient is continuous
 *   rotation term        sum over the effectors m in S(k), effector e, rot_weights[e] != 0, of
 *                          2 eff_w[m] rot_weights[e] a . v(R_m T_e^T),
 *                        v(M) = (M32 - M23, M13 - M31, M21 - M12): from
 *                        |R - T|_F^2 = |R|^2 - 2 tr(T^T R) + |T|^2 and dR / d theta = [a]x R;
 *                        T is used as given, orthonormal or not, and an effector of weight 0
 *                        never has its target read.
 * The angle term and the penalty are rounded as written, one product each and their sum, in
 * both arithmetics: a dimension with no effector (and, with the distance term, no node) below
 * it returns exactly that value.
 * Colliders: a fitness the collider term set to FLT_MAX stays FLT_MAX in out_fitness, and
 * out_gradient is always the gradient of the smooth terms above -- finite, and the same
 * whether or not the pose collides.  A caller polishing answers tests out_fitness.
 * The pose and aim terms of the folded kernels have no entry in
 * ikpso_solver_evaluate_frames and none here; for E = 1 the rotation term is
 * ikpso_solve_track_pose's with orientation_weight = rot_weights[0], as that entry documents.
 * FAST kernels on the hardware sin/cos scale the axes and the rotation R_m as
 * ikpso_solver_evaluate_jacobian and ikpso_solver_evaluate_frames do.
 * Served is every solver ikpso_solver_evaluate serves -- FAST and REFERENCE, masked chains,
 * folded DH arms through their Euler chain, trees, chains with colliders, every compiled
 * topology -- routed as evaluate routes it.  Nothing evaluate accepts is refused.
 * IKPSO_ERR_INVALID_ARG: what ikpso_solver_evaluate_frames rejects (a NULL solver; n < 0;
 * n > 0 with a NULL angles; a NaN, infinite or negative weight; some weight > 0 with a NULL
 * target_rot), and n > 0 with a NULL out_gradient.  n == 0 is IKPSO_OK with no device work.
 * Stream-ordered: the call does not synchronise, and it neither waits for nor settles a
 * pending solve. */
ikpso_status ikpso_solver_evaluate_gradient(ikpso_solver* solver, const float* angles, const float* targets,
                                            const float* rest, const float* target_rot, const float* rot_weights,
                                            int64_t n, float* out_fitness, float* out_gradient, void* stream);

/* Which node of given angle vectors hits which collider, on the device (added after ABI 5;
 * detect by symbol): the decisions behind a fitness of FLT_MAX -- the collider term makes them
 * per node and per collider and the fitness keeps only "some pair hit".  A planner scoring
 * poses learns which obstacle to route around, a caller whose answer came back FLT_MAX
 * whether the wrist or the elbow is stuck, a track caller at which frame and node contact
 * starts.
 *   angles         exactly ikpso_solver_evaluate_jacobian's: device, [n][D], the free
 *                  dimensions under an axis mask, locked axes at the chain's rotation, always
 *                  the Euler form of the chain.
 *   out_contacts   device, [n][C] uint32_t, C the collider_count of the descriptor the solver
 *                  was created with -- the caller's own indexing, the colliders the solver
 *                  left out as beyond the arm's reach (ikpso_solver_collider_count) included:
 *                  their columns are all zero.  Bit k - 1 of out_contacts[i][c] is set exactly
 *                  when node k's node box or link box is decided to intersect collider c at
 *                  vector i; J <= 20, so bits J .. 31 are 0.  Required when n > 0 and C > 0;
 *                  may be NULL when C == 0.
 *   out_positions  device, [n][J][3] or NULL: ikpso_solver_evaluate's positions (FAST: with
 *                  the caveat ikpso_solver_evaluate_frames states).
 * No targets, rest pose or weights: contacts depend on none of them.
 * Definition.  The boxes are the collider term's: the node box is a cube of edge 0.2 (the
 * reference's GIZMO_SIZE) at the node, the link box is length_k x 0.05 x 0.05 centred between
 * the node and its parent, both oriented by the node's world rotation R_k.  The decision is the
 * one the solver's own kernels make for this chain: REFERENCE decides by the reference's GJK,
 * bit for bit; FAST decides by the separating-axis test where its solve kernels do, and by GJK
 * where they do (a chain with an axis mask or with angle bounds beyond the hardware sin/cos
 * range, a generic tree, a collider whose quaternion is no rotation).  Every pair of a node and
 * a collider is decided -- nothing stops at a first hit -- and both boxes of a pair are OR-ed
 * into its bit.
 * Contract with ikpso_solver_evaluate, in both arithmetics and exactly: for the same solver
 * and angles and any targets, some word of out_contacts[i] is non-zero if and only if
 * out_fitness[i] == FLT_MAX.
 * Served is every solver ikpso_solver_evaluate serves, routed as evaluate routes it.  A
 * solver with no collider within reach (none given, or all left out) has nothing to decide:
 * out_contacts is zeroed in stream order and out_positions is ikpso_solver_evaluate's.
 * IKPSO_ERR_INVALID_ARG: a NULL solver; n < 0; n > 0 with a NULL angles; n > 0 and C > 0
 * with a NULL out_contacts.  n == 0 is IKPSO_OK with no device work.  Stream-ordered: the
 * call does not synchronise, and it neither waits for nor settles a pending solve. */
ikpso_status ikpso_solver_evaluate_contacts(ikpso_solver* solver, const float* angles, int64_t n,
                                            uint32_t* out_contacts, float* out_positions, void* stream);

/* Copy the generator states of local swarms [first_swarm, first_swarm + count)
 * (P states each, swarm-major, 48-byte curandState layout) into dst (any memory,
 * count * P states), after settling a pending solve (ABI >= 5).  Synchronises
 * `stream`.  The parity tests compare them with the oracle's: the draw count of
 * every particle (D at init, 3 D per iteration) is integer work, bit-exact. */
ikpso_status ikpso_solver_generator_states(ikpso_solver* solver, int64_t first_swarm, int64_t count, void* dst,
                                           void* stream);

/* Introspection.  dof = D, the free dimensions. */
int ikpso_solver_dof(const ikpso_solver* solver);
int ikpso_solver_effectors(const ikpso_solver* solver);
/* Colliders the solver's kernels test: those of the descriptor's colliders that lie
 * within the arm's reach of some node (one beyond it can never touch the arm, so it
 * can never change a fitness); with none left the chain is solved by the kernels
 * without the collider term.  The environment variable IKPSO_KEEP_FAR_COLLIDERS=1
 * keeps every collider. */
int ikpso_solver_collider_count(const ikpso_solver* solver);
/* Name of the kernel variant the solver dispatches to (family / topology); after a
 * solve_batch that AUTO routed to the cooperative latency variant (a few swarms),
 * that variant's name until the next solve (a long serial chain, whose chunks
 * are the latency width already, runs and names the cooperative kernel itself
 * there, whatever the number of swarms); after a solve_batch_until or a
 * solve_track that ran the streaming kernels for a cooperative solver, theirs. */
const char* ikpso_solver_kernel_name(const ikpso_solver* solver);

int ikpso_abi_version(void);
/* Hash of the sources the library was built from (csrc/ *.h *.hip *.cpp Makefile,
 * include/ *.h; ABI >= 5), plus "+" and a hash of the extra compiler flags of a
 * variant build.  The Python loader compares it with the tree it runs from. */
const char* ikpso_build_id(void);
const char* ikpso_status_string(ikpso_status status);
int ikpso_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* IKPSO_H */
