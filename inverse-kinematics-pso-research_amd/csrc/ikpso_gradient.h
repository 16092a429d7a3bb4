// ikpso_gradient.h -- the gradient kernel (ikpso_solver_evaluate_gradient).
//
//   k_evaluate_gradient: the fitness ikpso_solver_evaluate_frames reports and its derivative with respect
//     to every free angle, k_evaluate_frames' and k_evaluate_jacobian's sibling: the same builds, routing
//     and grid.  A forward pass (FitnessAcc), then one reverse sweep over the nodes that carries a wrench
//     from the leaves to the root: O(J) per vector whatever the number of effectors, no path table, no
//     stored Jacobian.
#pragma once

#include <hip/hip_runtime.h>

#include "ikpso_evaluate.h"

namespace ikpso {

// v(W T^T) = (M32 - M23, M13 - M31, M21 - M12) of M = W T^T, T row-major at q: the rows of W against the rows
// of T.  d|W - T|_F^2 / d theta = 2 a . v(W T^T) for dW / d theta = [a]x W, T orthonormal or not.
template <int MODE>
__device__ __forceinline__ Vec3 rot_torque(const Frame& W, const float* q)
{
    const Vec3 w1{W.r00, W.r01, W.r02}, w2{W.r10, W.r11, W.r12}, w3{W.r20, W.r21, W.r22};
    const Vec3 t1{q[0], q[1], q[2]}, t2{q[3], q[4], q[5]}, t3{q[6], q[7], q[8]};
    return Vec3{dot3<MODE>(w3, t2) - dot3<MODE>(w2, t3), dot3<MODE>(w1, t3) - dot3<MODE>(w3, t1),
                dot3<MODE>(w2, t1) - dot3<MODE>(w1, t2)};
}

// The part of one free angle's derivative that needs no frame: the angle term 2 aw (x - rest) and the
// soft-limit penalty's 2 lw (x - hi) above the soft bound, -2 lw (lo - x) below it, 0 between and at the
// bounds (the larger excess where the bounds cross, as the fitness takes it).  Never contracted, in either
// arithmetic: a dimension with no effector below it returns exactly this value.
__device__ __forceinline__ float local_gradient(float x, float rest, float aw2, bool penalty, float lw2,
                                                const float* slo, const float* shi)
{
#pragma clang fp contract(off)
    float g = aw2 * (x - rest);
    if (penalty) {
        const float up = x - *shi, dn = *slo - x;
        if (fmaxf(up, dn) > 0.0f) g = g + (up >= dn ? lw2 * up : -(lw2 * dn));
    }
    return g;
}

// One lane per angle vector, grid-stride, k_evaluate_frames' inputs.
// Forward: FitnessAcc::node composes the frames F[k] and the fitness sums, finish() gives the fitness, and
// the rotation error is formed node by node on the rotation k_evaluate_frames reports (compensated on the
// transcendental unit's builds), in its order: out_fitness is that entry's.  The same loop seeds node k's
// wrench about the origin's position o -- a force and a moment:
//   g   = 2 eff_w (p_k - t_k) + 2 dw (p_k - ref_k)          (effector term, distance term)
//   f_k = g,   m_k = (p_k - o) x g + 2 eff_w rw v(R_k T^T)   (rotation term; v as rot_torque)
// Reverse: k = J .. 1 (parent[k] < k, so every child of k has been added into k's wrench by then).  With
// q = p_parent(k) the node's three world axes a_c (k_evaluate_jacobian's: the parent's first column, its
// second and third turned by the node's own Rx, the node's third column) give
//   d fitness / d angle c of node k = a_c . (m_k - (q - o) x f_k) + local_gradient,
// since sum_m g_m . (a x (p_m - q)) = a . (sum_m (p_m - o) x g_m - (q - o) x sum_m g_m) over the subtree;
// then the wrench is added into the parent's.  The compiled topologies resolve the parent at compile time
// and keep the wrenches in registers; the generic trees index them at run time, in scratch beside their
// frames.
// The collider term only ever replaces the fitness by FLT_MAX: the gradient is that of the smooth terms,
// colliding or not.
// The builds on the transcendental unit's sin/cos scale the axes as k_evaluate_jacobian does
// (GradientIO::frame_comp, axis_y_comp), so |a| = 1 to float32 rounding.
// Stores are one lane per vector ([n][DF] is strided across the wave), as in the siblings.
template <class Topo, int MODE, int TERMS>
__global__ void __launch_bounds__(256) k_evaluate_gradient(const ChainConsts<Topo::J> cc, const GradientIO gio)
{
    constexpr int J = Topo::J;
    constexpr int D = Topo::D;
    constexpr int HW = kHwTrig<Topo, MODE, TERMS>;
    constexpr bool kComp = HW == kTrigHw || HW == kTrigHwRev;
    static_assert(!Topo::kDH && J <= kMaxEffFrames, "the Euler topologies; a weight slot for every node");
    static_assert(!(TERMS & kTermRev), "angles in radians, frames in world coordinates: the evaluate builds");
    const int64_t DF = cc.dfree;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < gio.n;
         n += (int64_t)gridDim.x * blockDim.x) {
        float x[D], rest[D], tgt[3 * J];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const bool fr = dim_free(cc, d);
            const int64_t r = n * DF + dim_rank(cc, d);
            x[d] = fr ? gio.angles[r] : cc.rest[d];
            rest[d] = gio.rest && fr ? gio.rest[r] : cc.rest[d];
        }
        if (gio.targets) {
#pragma unroll
            for (int k = 1; k <= J; ++k) {
                const int s = cc.eff_slot[k];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    tgt[3 * (k - 1) + c] = s >= 0 ? gio.targets[(n * cc.num_eff + s) * 3 + c] : 0.0f;
            }
        } else {
#pragma unroll
            for (int d = 0; d < 3 * J; ++d) tgt[d] = cc.tgt0[d];
        }
        CandBuf<Topo, TERMS> cb;
        FitnessAcc<Topo, MODE, TERMS> acc(cc, nullptr, cc.aux + 4 * J, cb.v);
#pragma unroll
        for (int k = 1; k <= J; ++k)
            acc.node(cc, k, x + 3 * (k - 1), rest + 3 * (k - 1), tgt + 3 * (k - 1), nullptr);
        float f = acc.finish(cc);
        // the rotation error (k_evaluate_frames' order) and every node's own wrench
        const Vec3 o{acc.F[0].px, acc.F[0].py, acc.F[0].pz};
        const float dw2 = 2.0f * cc.dw_j;
        Vec3 wf[J + 1], wm[J + 1];
        wf[0] = wm[0] = Vec3{0.0f, 0.0f, 0.0f};
        float orient = 0.0f;
#pragma unroll
        for (int k = 1; k <= J; ++k) {
            const Vec3 p{acc.F[k].px, acc.F[k].py, acc.F[k].pz};
            Vec3 g{0.0f, 0.0f, 0.0f}, torque{0.0f, 0.0f, 0.0f};
            const float ew = cc.eff_w[k];
            if (Topo::effector(k) && ew != 0.0f) {  // uniform (a generic tree's node that is no effector: 0)
                const Vec3 t{tgt[3 * (k - 1) + 0], tgt[3 * (k - 1) + 1], tgt[3 * (k - 1) + 2]};
                g = axpy3<MODE>(g, 2.0f * ew, sub3(p, t));
            }
            if (acc.posref) {
                const float* pr = cc.aux + 4 * (k - 1);
                g = axpy3<MODE>(g, dw2, sub3(p, Vec3{pr[0], pr[1], pr[2]}));
            }
            const int s = cc.eff_slot[k];
            if (Topo::effector(k) && s >= 0 && gio.target_rot) {
                float rw = 0.0f;
#pragma unroll
                for (int e = 0; e < kMaxEffFrames; ++e) rw = s == e ? gio.rot_w[e] : rw;
                if (rw > 0.0f) {  // a weight of 0 never reads its target
                    Frame W = acc.F[k];
                    if constexpr (kComp) scale_up(W, gio.frame_comp[k - 1]);
                    const float* q = gio.target_rot + (n * cc.num_eff + s) * 9;
                    const float e2 = frame_rot_error<MODE>(W, q);
                    if constexpr (MODE == IKPSO_ARITH_REFERENCE) {
#pragma clang fp contract(off)
                        orient = orient + (ew * rw) * e2;
                    } else {
#pragma clang fp contract(fast)
                        orient = orient + (ew * rw) * e2;
                    }
                    torque = axpy3<MODE>(torque, 2.0f * (ew * rw), rot_torque<MODE>(W, q));
                }
            }
            wf[k] = g;
            wm[k] = add3(cross3<MODE>(sub3(p, o), g), torque);
        }
        f = add_last<TERMS>(f, orient);
        if (gio.out_fitness) gio.out_fitness[n] = f;
        // the reverse sweep
        const float aw2 = 2.0f * angle_weight<TERMS>(cc), lw2 = 2.0f * limit_weight<TERMS>(cc);
        float* const out = gio.out_gradient + n * DF;
#pragma unroll
        for (int k = J; k >= 1; --k) {
            const int pk = Topo::kGeneric ? cc.parent[k] : Topo::parent(k);
            const uint32_t fm = (uint32_t)(cc.free_mask >> (3 * (k - 1))) & 7u;
            const Vec3 fk = wf[k], mk = wm[k];
            if (fm != 0u) {  // a locked node has no columns (uniform)
                const Frame P = acc.F[pk];
                float sa, ca;
                if constexpr (MODE == IKPSO_ARITH_REFERENCE)
                    sincos_reference(x[3 * (k - 1)], &sa, &ca);
                else
                    sincos_fast<HW>(x[3 * (k - 1)], &sa, &ca);
                Vec3 a[3];
                a[0] = Vec3{P.r00, P.r10, P.r20};
                if constexpr (MODE == IKPSO_ARITH_REFERENCE) {
#pragma clang fp contract(off)
                    a[1] = Vec3{P.r01 * ca + P.r02 * sa, P.r11 * ca + P.r12 * sa, P.r21 * ca + P.r22 * sa};
                } else {
#pragma clang fp contract(fast)
                    a[1] = Vec3{P.r01 * ca + P.r02 * sa, P.r11 * ca + P.r12 * sa, P.r21 * ca + P.r22 * sa};
                }
                a[2] = Vec3{acc.F[k].r02, acc.F[k].r12, acc.F[k].r22};
                if constexpr (kComp) {
                    // the origin's frame is the chain's own, not this unit's: nothing to add back
                    float cx = 0.0f;
#pragma unroll
                    for (int q = 1; q <= J; ++q) cx = pk == q ? gio.frame_comp[q - 1] : cx;
                    const float comp[3] = {cx, gio.axis_y_comp[k - 1], gio.frame_comp[k - 1]};
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        a[c].x = __builtin_fmaf(a[c].x, comp[c], a[c].x);
                        a[c].y = __builtin_fmaf(a[c].y, comp[c], a[c].y);
                        a[c].z = __builtin_fmaf(a[c].z, comp[c], a[c].z);
                    }
                }
                // the subtree's moment about the pivot q = p_parent(k)
                const Vec3 tq = sub3(mk, cross3<MODE>(sub3(Vec3{P.px, P.py, P.pz}, o), fk));
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (!((fm >> c) & 1u)) continue;
                    const int d = 3 * (k - 1) + c;
                    const float loc = local_gradient(x[d], rest[d], aw2, acc.penalty, lw2, acc.soft + d, acc.soft + 3 * J + d);
                    out[dim_rank(cc, d)] = dot3<MODE>(a[c], tq) + loc;
                }
            }
            wf[pk] = add3(wf[pk], fk);
            wm[pk] = add3(wm[pk], mk);
        }
    }
}

// ikpso_solver_evaluate_gradient's evaluator kind (run_evaluate_kind).
struct EvalGradient : EvalAxes<GradientIO> {
    template <class Topo, int MODE, int TERMS>
    static constexpr auto kernel() { return &k_evaluate_gradient<Topo, MODE, TERMS>; }
};

}  // namespace ikpso
