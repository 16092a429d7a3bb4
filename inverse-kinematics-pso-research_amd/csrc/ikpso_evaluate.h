// ikpso_evaluate.h -- the evaluate family: kernels that take given angle vectors, one lane per vector
// (templates; instantiated per topology in ikpso_inst_*.hip), and the one launch path they share.
//
//   k_evaluate: FK + fitness of given angle vectors (parity/KAT entry).
//   k_evaluate_frames: the same with the node rotations, the rotation error per effector and the
//     rotation term in the fitness (ikpso_solver_evaluate_frames).
//   k_evaluate_jacobian (ikpso_jacobian.h), k_evaluate_gradient (ikpso_gradient.h) and k_evaluate_contacts
//     (ikpso_contacts.h) build on this header.
//
// All four run the same builds on the same grid (launch_evaluate_build).  The three with units of their
// own go through run_evaluate_kind: an evaluator kind names its parameter block and its kernel.
#pragma once

#include <hip/hip_runtime.h>

#include "ikpso_device.h"
#include "ikpso_kernels.h"

namespace ikpso {

// ---------------------------------------------------------------- shared steps
// Each is written once, in the floating-point order the kernels had it: REFERENCE compiles without FMA
// contraction, so the written order is the rounding.

// The rotation of W scaled up by c, its position untouched: what the builds on the transcendental unit's
// sin/cos add back to a node's rotation (EvalFramesIO::rot_comp).
__device__ __forceinline__ void scale_up(Frame& W, float c)
{
    W.r00 = __builtin_fmaf(W.r00, c, W.r00), W.r01 = __builtin_fmaf(W.r01, c, W.r01);
    W.r02 = __builtin_fmaf(W.r02, c, W.r02), W.r10 = __builtin_fmaf(W.r10, c, W.r10);
    W.r11 = __builtin_fmaf(W.r11, c, W.r11), W.r12 = __builtin_fmaf(W.r12, c, W.r12);
    W.r20 = __builtin_fmaf(W.r20, c, W.r20), W.r21 = __builtin_fmaf(W.r21, c, W.r21);
    W.r22 = __builtin_fmaf(W.r22, c, W.r22);
}

// The rotation term is added last; a fitness the collider block set to FLT_MAX stays FLT_MAX.
template <int TERMS>
__device__ __forceinline__ float add_last(float f, float orient)
{
    if (!((TERMS & kTermColliders) && f == FLT_MAX)) f = f + orient;
    return f;
}

struct Vec3 {
    float x, y, z;
};

// a x b and a . b
template <int MODE>
__device__ __forceinline__ Vec3 cross3(const Vec3& a, const Vec3& b)
{
    if constexpr (MODE == IKPSO_ARITH_REFERENCE) {
#pragma clang fp contract(off)
        return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
    } else {
#pragma clang fp contract(fast)
        return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
    }
}
template <int MODE>
__device__ __forceinline__ float dot3(const Vec3& a, const Vec3& b)
{
    if constexpr (MODE == IKPSO_ARITH_REFERENCE) {
#pragma clang fp contract(off)
        return (a.x * b.x + a.y * b.y) + a.z * b.z;
    } else {
#pragma clang fp contract(fast)
        return (a.x * b.x + a.y * b.y) + a.z * b.z;
    }
}
// a + s b
template <int MODE>
__device__ __forceinline__ Vec3 axpy3(const Vec3& a, float s, const Vec3& b)
{
    if constexpr (MODE == IKPSO_ARITH_REFERENCE) {
#pragma clang fp contract(off)
        return Vec3{a.x + s * b.x, a.y + s * b.y, a.z + s * b.z};
    } else {
#pragma clang fp contract(fast)
        return Vec3{a.x + s * b.x, a.y + s * b.y, a.z + s * b.z};
    }
}
__device__ __forceinline__ Vec3 sub3(const Vec3& a, const Vec3& b) { return Vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec3 add3(const Vec3& a, const Vec3& b) { return Vec3{a.x + b.x, a.y + b.y, a.z + b.z}; }

// ----------------------------------------------------------- evaluate kernel
// angles, rest: [n][dfree] over the free dimensions (locked ones at the chain's rest).
template <class Topo, int MODE, int TERMS>
__global__ void __launch_bounds__(256) k_evaluate(const ChainConsts<Topo::J> cc, EvalIO io)
{
    constexpr int J = Topo::J;
    constexpr int D = Topo::D;
    const int64_t DF = cc.dfree;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < io.n;
         n += (int64_t)gridDim.x * blockDim.x) {
        float x[D], rest[D], tgt[3 * J], pos[3 * J];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const bool fr = dim_free(cc, d);
            const int64_t r = n * DF + dim_rank(cc, d);
            x[d] = fr ? io.angles[r] : cc.rest[d];
            rest[d] = io.rest && fr ? io.rest[r] : cc.rest[d];
        }
        if (io.targets) {
#pragma unroll
            for (int k = 1; k <= J; ++k) {
                const int s = cc.eff_slot[k];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    tgt[3 * (k - 1) + c] = s >= 0 ? io.targets[(n * cc.num_eff + s) * 3 + c] : 0.0f;
            }
        } else {
#pragma unroll
            for (int d = 0; d < 3 * J; ++d) tgt[d] = cc.tgt0[d];
        }
        const float f = fitness<Topo, MODE, TERMS>(cc, x, rest, tgt, pos, nullptr, cc.aux + 4 * J);
        if (io.out_fitness) io.out_fitness[n] = f;
        if (io.out_positions) {
#pragma unroll
            for (int d = 0; d < 3 * J; ++d) io.out_positions[n * 3 * J + d] = pos[d];
        }
    }
}

// |R - T|_F^2 of a frame's rotation against a row-major target: the nine squared differences
// accumulated in row-major order.  REFERENCE: no FMA contraction, so the order is the rounding.
template <int MODE>
__device__ __forceinline__ float frame_rot_error(const Frame& W, const float* q)
{
    const float d0 = W.r00 - q[0], d1 = W.r01 - q[1], d2 = W.r02 - q[2];
    const float d3 = W.r10 - q[3], d4 = W.r11 - q[4], d5 = W.r12 - q[5];
    const float d6 = W.r20 - q[6], d7 = W.r21 - q[7], d8 = W.r22 - q[8];
    if constexpr (MODE == IKPSO_ARITH_REFERENCE) {
#pragma clang fp contract(off)
        return (((((((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3) + d4 * d4) + d5 * d5) + d6 * d6) + d7 * d7) + d8 * d8;
    } else {
#pragma clang fp contract(fast)
        return (((((((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3) + d4 * d4) + d5 * d5) + d6 * d6) + d7 * d7) + d8 * d8;
    }
}

// k_evaluate's sibling (ikpso_solver_evaluate_frames): the same inputs, builds and routing, and the
// rotations of the node frames FitnessAcc composes (F[k]: whole in the leaves' closed form too) kept --
// written out, measured against a rotation target per effector, and that term added to the fitness
// last.  A kernel of its own, so k_evaluate keeps its code.  Stores are one lane per vector ([n][J][9]
// is strided across the wave).
// The builds on the transcendental unit's sin/cos report node k's rotation scaled up by 2 depth(k) eps
// (EvalFramesIO::rot_comp): every plane rotation built from that unit's pairs shrinks the two columns it mixes
// by eps (kHwTrigAmplitudeBias), and each column is mixed by two of a node's three rotations, so the columns
// of F[k] are short by exactly that factor -- 2.6e-6 in R R^T at depth 20.  The same compensation the link
// lengths carry (len_hw), here exact per column rather than in the mean.  The rotation error and the term
// are formed on the compensated rotation, the one the caller gets.  FitnessAcc, and so the fitness without
// the term and the positions, are untouched.
template <class Topo, int MODE, int TERMS>
__global__ void __launch_bounds__(256) k_evaluate_frames(const ChainConsts<Topo::J> cc, const EvalFramesIO fio)
{
    constexpr int J = Topo::J;
    constexpr int D = Topo::D;
    static_assert(!Topo::kDH && J <= kMaxEffFrames, "the Euler topologies; a weight slot for every node");
    const EvalIO& io = fio.e;
    const int64_t DF = cc.dfree;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < io.n;
         n += (int64_t)gridDim.x * blockDim.x) {
        float x[D], rest[D], tgt[3 * J], pos[3 * J];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const bool fr = dim_free(cc, d);
            const int64_t r = n * DF + dim_rank(cc, d);
            x[d] = fr ? io.angles[r] : cc.rest[d];
            rest[d] = io.rest && fr ? io.rest[r] : cc.rest[d];
        }
        if (io.targets) {
#pragma unroll
            for (int k = 1; k <= J; ++k) {
                const int s = cc.eff_slot[k];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    tgt[3 * (k - 1) + c] = s >= 0 ? io.targets[(n * cc.num_eff + s) * 3 + c] : 0.0f;
            }
        } else {
#pragma unroll
            for (int d = 0; d < 3 * J; ++d) tgt[d] = cc.tgt0[d];
        }
        // fitness<Topo, MODE, TERMS> with node positions (the forward form), the accumulator kept
        CandBuf<Topo, TERMS> cb;
        FitnessAcc<Topo, MODE, TERMS> acc(cc, nullptr, cc.aux + 4 * J, cb.v);
#pragma unroll
        for (int k = 1; k <= J; ++k) acc.node(cc, k, x + 3 * (k - 1), rest + 3 * (k - 1), tgt + 3 * (k - 1), pos);
        float f = acc.finish(cc);
        float orient = 0.0f;
#pragma unroll
        for (int k = 1; k <= J; ++k) {
            Frame W = acc.F[k];
            constexpr int HW = kHwTrig<Topo, MODE, TERMS>;
            if constexpr (HW == kTrigHw || HW == kTrigHwRev) scale_up(W, fio.rot_comp[k - 1]);
            if (fio.out_rotations) {
                float* o = fio.out_rotations + (n * J + (k - 1)) * 9;
                o[0] = W.r00, o[1] = W.r01, o[2] = W.r02;
                o[3] = W.r10, o[4] = W.r11, o[5] = W.r12;
                o[6] = W.r20, o[7] = W.r21, o[8] = W.r22;
            }
            const int s = cc.eff_slot[k];
            if (Topo::effector(k) && s >= 0 && fio.target_rot) {
                // the caller's weight by constant indices (stage_swarm_frames); uniform, like s
                float rw = 0.0f;
#pragma unroll
                for (int e = 0; e < kMaxEffFrames; ++e) rw = s == e ? fio.rot_w[e] : rw;
                // a weight of 0 reads its target for out_rot_error alone, never into the sum
                if (rw > 0.0f || fio.out_rot_error) {
                    const float e2 = frame_rot_error<MODE>(W, fio.target_rot + (n * cc.num_eff + s) * 9);
                    if (fio.out_rot_error) fio.out_rot_error[n * cc.num_eff + s] = e2;
                    if (rw > 0.0f) {
                        if constexpr (MODE == IKPSO_ARITH_REFERENCE) {
#pragma clang fp contract(off)
                            orient = orient + (cc.eff_w[k] * rw) * e2;
                        } else {
#pragma clang fp contract(fast)
                            orient = orient + (cc.eff_w[k] * rw) * e2;
                        }
                    }
                }
            }
        }
        f = add_last<TERMS>(f, orient);
        if (io.out_fitness) io.out_fitness[n] = f;
        if (io.out_positions) {
#pragma unroll
            for (int d = 0; d < 3 * J; ++d) io.out_positions[n * 3 * J + d] = pos[d];
        }
    }
}

// --------------------------------------------------------------- dispatch
// The evaluate kernels' launch for n vectors: launch(term set, grid, threads) of the build that evaluates
// the chain.  The mask only places the given angles (no PSO): the unmasked builds evaluate it -- but a chain
// whose angles reach beyond the transcendental unit's range (poly_trig) is solved by the masked collider
// builds for their polynomial sin/cos, and is evaluated by the same arithmetic (as one with colliders that
// are no rotations).
template <class F>
inline hipError_t launch_evaluate_build(const ChainHost& ch, int64_t n, F&& launch)
{
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks), threads(256);
    if ((ch.poly_trig && IKPSO_COLLIDE_HW_TRIG) || (ch.num_coll > 0 && !ch.coll_obb))
        launch(std::integral_constant<int, kTermRuntime | kTermColliders | kTermMask>{}, grid, threads);
    else if (ch.num_coll > 0)
        launch(std::integral_constant<int, kTermRuntime | kTermColliders>{}, grid, threads);
    else
        launch(std::integral_constant<int, kTermRuntime>{}, grid, threads);
    return hipGetLastError();
}

template <class Topo, int MODE>
inline hipError_t run_evaluate(const ChainHost& ch, const EvalIO& io, hipStream_t stream)
{
    if constexpr (Topo::kDH) {  // the solver evaluates through its Euler chain
        return hipErrorNotSupported;
    } else {
        const ChainConsts<Topo::J> cc = make_consts<Topo::J>(ch);
        return launch_evaluate_build(ch, io.n, [&](auto t, dim3 grid, dim3 threads) {
            hipLaunchKernelGGL((k_evaluate<Topo, MODE, decltype(t)::value>), grid, threads, 0, stream, cc, io);
        });
    }
}
// What the builds on the transcendental unit's sin/cos add back (kHwTrigAmplitudeBias; fp64, rounded once),
// at k - 1: frame_comp (null: not wanted) is 2 depth(k) eps, for a column of node k's frame; axis_y_comp (null too) is
// (2 depth(k) - 1) eps, for node k's y axis, a column of the parent's frame turned by the node's Rx alone.
template <int J>
inline void fill_trig_comp(const ChainHost& ch, float* frame_comp, float* axis_y_comp)
{
    int depth[J + 1];
    node_depths<J>(ch, depth);
    for (int k = 1; k <= J; ++k) {
        if (frame_comp) frame_comp[k - 1] = (float)(2.0 * depth[k] * kHwTrigAmplitudeBias);
        if (axis_y_comp) axis_y_comp[k - 1] = (float)((2.0 * depth[k] - 1.0) * kHwTrigAmplitudeBias);
    }
}

// An evaluator kind (EvalOps' Kind) names its parameter block IO, where that block holds the vector count
// and the compensation arrays, and its kernel; kPlainBuild, whether it has a kernel for a chain without the
// collider term (one that has none refuses such a chain: nothing of it is instantiated for the plain term
// set).  EvalFrames: ikpso_solver_evaluate_frames; EvalJacobian and EvalGradient stand beside their kernels,
// on EvalAxes; EvalContacts beside its own (ikpso_contacts.h).
struct EvalFrames {
    using IO = EvalFramesIO;
    static constexpr bool kPlainBuild = true;
    static int64_t n(const IO& io) { return io.e.n; }
    static float* frame_comp(IO& io) { return io.rot_comp; }
    static float* axis_y_comp(IO&) { return nullptr; }
    template <class Topo, int MODE, int TERMS>
    static constexpr auto kernel() { return &k_evaluate_frames<Topo, MODE, TERMS>; }
};
template <class AxesIO>
struct EvalAxes {  // the parameter blocks with JacobianIO's joint-axis compensation
    using IO = AxesIO;
    static constexpr bool kPlainBuild = true;
    static int64_t n(const IO& io) { return io.n; }
    static float* frame_comp(IO& io) { return io.frame_comp; }
    static float* axis_y_comp(IO& io) { return io.axis_y_comp; }
};

// run_evaluate's grid and routing rule on Kind's kernel, the compensation filled into a copy of the
// caller's parameters.
template <class Kind, class Topo, int MODE>
inline hipError_t run_evaluate_kind(const ChainHost& ch, const typename Kind::IO& caller_io, hipStream_t stream)
{
    static_assert(!Topo::kDH, "the solver evaluates through its Euler chain");
    const ChainConsts<Topo::J> cc = make_consts<Topo::J>(ch);
    typename Kind::IO io = caller_io;
    fill_trig_comp<Topo::J>(ch, Kind::frame_comp(io), Kind::axis_y_comp(io));
    bool refused = false;
    const hipError_t err = launch_evaluate_build(ch, Kind::n(io), [&](auto t, dim3 grid, dim3 threads) {
        constexpr int TERMS = decltype(t)::value;
        if constexpr (Kind::kPlainBuild || (TERMS & kTermColliders))
            hipLaunchKernelGGL((Kind::template kernel<Topo, MODE, TERMS>()), grid, threads, 0, stream, cc, io);
        else
            refused = true;
    });
    return refused ? hipErrorNotSupported : err;
}

}  // namespace ikpso
