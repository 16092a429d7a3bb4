// ikpso_jacobian.h -- the Jacobian kernel (ikpso_solver_evaluate_jacobian).
//
//   k_evaluate_jacobian: FK of given angle vectors and the geometric Jacobian of every effector,
//     k_evaluate_frames' sibling: the same builds, routing and grid, derivatives where that one has
//     rotation errors.  No fitness, targets, rest pose or weights: the Jacobian depends on none of them.
#pragma once

#include <hip/hip_runtime.h>

#include "ikpso_evaluate.h"

namespace ikpso {

// Is node k node m or one of its ancestors?  (The compiled topologies: folded at compile time.)
template <class Topo>
__host__ __device__ constexpr bool on_path(int k, int m)
{
    for (int a = m; a > 0; a = Topo::parent(a))
        if (a == k) return true;
    return false;
}

// The generic trees' path table, staged in LDS once per workgroup (their parent table is run-time data, and
// the effector loop below runs over a run-time node index): path[m] has bit k - 1 set when node k is m or
// an ancestor of m, slot[m] is m's effector ordinal or -1.
template <int J>
struct PathTable {
    uint32_t path[J + 1];
    int32_t slot[J + 1];
};

// The three world axes of node k's angles, scaled by `comp` where the build compensates (see the kernel).
struct JointAxes {
    float a[3][3];  // [angle][x y z]
};

// One effector's columns of node k's free angles: (a x d, a) with d = p_m - p_parent(k), or +0.  o points at
// the effector's [6][DF] block, fm has bit c set when angle c of the node is free.
// REFERENCE: no FMA contraction, so the written order is the rounding.
template <int MODE, class CC>
__device__ __forceinline__ void store_columns(const CC& cc, float* o, int64_t DF, int k, uint32_t fm, bool on,
                                              const JointAxes& ax, float dx, float dy, float dz)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (!((fm >> c) & 1u)) continue;
        const float a0 = ax.a[c][0], a1 = ax.a[c][1], a2 = ax.a[c][2];
        const Vec3 l = cross3<MODE>(Vec3{a0, a1, a2}, Vec3{dx, dy, dz});
        float* q = o + dim_rank(cc, 3 * (k - 1) + c);
        q[0 * DF] = on ? l.x : 0.0f;
        q[1 * DF] = on ? l.y : 0.0f;
        q[2 * DF] = on ? l.z : 0.0f;
        q[3 * DF] = on ? a0 : 0.0f;
        q[4 * DF] = on ? a1 : 0.0f;
        q[5 * DF] = on ? a2 : 0.0f;
    }
}

// One lane per angle vector, grid-stride.  The forward pass is FitnessAcc's (the frames F[k] and the node
// positions of the build that evaluates the chain; its fitness sums are never finished, so the compiler
// drops them).  The second pass takes, node by node, the world axes of the node's three angles
//   x: R_parent e_x           the parent frame's first column
//   y: R_parent Rx(x_k) e_y   its second and third columns turned by the node's own Rx
//   z: R_k e_z                the node frame's third column (Rz leaves it alone)
// and writes the column (a x (p_m - p_parent(k)), a) of every effector m below the node, +0 for every
// other effector.  The compiled topologies resolve "below" at compile time (on_path); the generic trees
// read it from the staged PathTable in a run-time loop over the nodes, which keeps their code size linear
// in J (their frames live in scratch already).
// The builds on the transcendental unit's sin/cos scale the axes up by the known shrink of that unit's
// plane rotations, as k_evaluate_frames scales the rotation it reports (JacobianIO::frame_comp,
// axis_y_comp), so |a| = 1 to float32 rounding; the positions are untouched.
// Stores are one lane per vector ([n][E][6][DF] is strided across the wave), as in k_evaluate_frames.
template <class Topo, int MODE, int TERMS>
__global__ void __launch_bounds__(256) k_evaluate_jacobian(const ChainConsts<Topo::J> cc, const JacobianIO jio)
{
    constexpr int J = Topo::J;
    constexpr int D = Topo::D;
    constexpr int HW = kHwTrig<Topo, MODE, TERMS>;
    constexpr bool kComp = HW == kTrigHw || HW == kTrigHwRev;
    static_assert(!Topo::kDH && J <= kMaxEffFrames, "the Euler topologies; a compensation slot for every node");
    const int64_t DF = cc.dfree;
    const int64_t E = cc.num_eff;
    __shared__ PathTable<Topo::kGeneric ? J : 0> tab;
    if constexpr (Topo::kGeneric) {
        if (threadIdx.x == 0) {
            tab.path[0] = 0u;
            tab.slot[0] = -1;
#pragma unroll
            for (int k = 1; k <= J; ++k) {
                tab.path[k] = tab.path[cc.parent[k]] | (1u << (k - 1));  // parent[k] < k (parse_chain)
                tab.slot[k] = cc.eff_slot[k];
            }
        }
        __syncthreads();
    }
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < jio.n;
         n += (int64_t)gridDim.x * blockDim.x) {
        float x[D], pos[3 * J];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = dim_free(cc, d) ? jio.angles[n * DF + dim_rank(cc, d)] : cc.rest[d];
        // the forward pass (rest = x and a target nobody reads: the sums are dead)
        CandBuf<Topo, TERMS> cb;
        FitnessAcc<Topo, MODE, TERMS> acc(cc, nullptr, cc.aux + 4 * J, cb.v);
#pragma unroll
        for (int k = 1; k <= J; ++k) acc.node(cc, k, x + 3 * (k - 1), x + 3 * (k - 1), x + 3 * (k - 1), pos);
        if (jio.out_positions) {
#pragma unroll
            for (int d = 0; d < 3 * J; ++d) jio.out_positions[n * 3 * J + d] = pos[d];
        }
        float* const out = jio.out_jacobian + n * E * 6 * DF;
#pragma unroll
        for (int k = 1; k <= J; ++k) {
            const uint32_t fm = (uint32_t)(cc.free_mask >> (3 * (k - 1))) & 7u;
            if (fm == 0u) continue;  // a locked node has no columns (uniform)
            const int pk = Topo::kGeneric ? cc.parent[k] : Topo::parent(k);
            const Frame P = acc.F[pk];
            float sa, ca;
            if constexpr (MODE == IKPSO_ARITH_REFERENCE)
                sincos_reference(x[3 * (k - 1)], &sa, &ca);
            else
                sincos_fast<HW>(x[3 * (k - 1)], &sa, &ca);
            JointAxes ax;
            ax.a[0][0] = P.r00, ax.a[0][1] = P.r10, ax.a[0][2] = P.r20;
            if constexpr (MODE == IKPSO_ARITH_REFERENCE) {
#pragma clang fp contract(off)
                ax.a[1][0] = P.r01 * ca + P.r02 * sa;
                ax.a[1][1] = P.r11 * ca + P.r12 * sa;
                ax.a[1][2] = P.r21 * ca + P.r22 * sa;
            } else {
#pragma clang fp contract(fast)
                ax.a[1][0] = P.r01 * ca + P.r02 * sa;
                ax.a[1][1] = P.r11 * ca + P.r12 * sa;
                ax.a[1][2] = P.r21 * ca + P.r22 * sa;
            }
            ax.a[2][0] = acc.F[k].r02, ax.a[2][1] = acc.F[k].r12, ax.a[2][2] = acc.F[k].r22;
            if constexpr (kComp) {
                // the origin's frame is the chain's own, not this unit's: nothing to add back
                float cx = 0.0f;
#pragma unroll
                for (int q = 1; q <= J; ++q) cx = pk == q ? jio.frame_comp[q - 1] : cx;
                const float cy = jio.axis_y_comp[k - 1], cz = jio.frame_comp[k - 1];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    ax.a[0][i] = __builtin_fmaf(ax.a[0][i], cx, ax.a[0][i]);
                    ax.a[1][i] = __builtin_fmaf(ax.a[1][i], cy, ax.a[1][i]);
                    ax.a[2][i] = __builtin_fmaf(ax.a[2][i], cz, ax.a[2][i]);
                }
            }
            if constexpr (Topo::kGeneric) {
#pragma unroll 1
                for (int m = 1; m <= J; ++m) {
                    const int s = tab.slot[m];
                    if (s < 0) continue;
                    const bool on = (tab.path[m] >> (k - 1)) & 1u;
                    const Frame& M = acc.F[m];
                    store_columns<MODE>(cc, out + s * 6 * DF, DF, k, fm, on, ax, M.px - P.px, M.py - P.py,
                                        M.pz - P.pz);
                }
            } else {
#pragma unroll
                for (int m = 1; m <= J; ++m) {
                    if (!Topo::effector(m)) continue;
                    const int s = cc.eff_slot[m];
                    if (s < 0) continue;
                    store_columns<MODE>(cc, out + s * 6 * DF, DF, k, fm, on_path<Topo>(k, m), ax,
                                        pos[3 * (m - 1) + 0] - P.px, pos[3 * (m - 1) + 1] - P.py,
                                        pos[3 * (m - 1) + 2] - P.pz);
                }
            }
        }
    }
}

// ikpso_solver_evaluate_jacobian's evaluator kind (run_evaluate_kind).
struct EvalJacobian : EvalAxes<JacobianIO> {
    template <class Topo, int MODE, int TERMS>
    static constexpr auto kernel() { return &k_evaluate_jacobian<Topo, MODE, TERMS>; }
};

}  // namespace ikpso
