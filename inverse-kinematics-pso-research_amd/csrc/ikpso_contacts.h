// ikpso_contacts.h -- the contacts kernel (ikpso_solver_evaluate_contacts).
//
//   k_evaluate_contacts: which node of given angle vectors hits which collider -- the decisions the
//     collider term of the fitness makes and throws away after the first hit, all of them kept.
//     k_evaluate_jacobian's sibling: the same angle vectors, builds, routing and grid; no fitness, targets,
//     rest pose or weights (contacts depend on none of them).  Collider term sets only: a chain with no
//     collider has nothing to decide (EvalContacts::kPlainBuild).
#pragma once

#include <hip/hip_runtime.h>

#include "ikpso_evaluate.h"

namespace ikpso {

// One lane per angle vector, grid-stride.  The forward pass is FitnessAcc's, so the frames, the inline sphere
// test and the frames kept for the near nodes are those k_evaluate's fitness decides on: REFERENCE compiles
// without contraction and the FAST collider builds pin every rounding (FitnessAcc::kPin), so a frame does not
// depend on the kernel that composes it.  Then, per near node, the boxes in the build's own form --
// finish_for_update's, statement for statement: the compact candidate's third axis and parent position
// rebuilt where kCompactCand, the stored frame otherwise -- through the reporting siblings of the build's box
// test (node_contacts_obb where kFastSat, node_contacts -- GJK -- otherwise).  The generic trees test a near
// node inside the pass and stop at the first hit (FitnessAcc::hit, unused here); their near test is run
// again after the pass, on acc.F[k], for every node.
// Hence: some word of a vector is non-zero exactly when k_evaluate's fitness of it is FLT_MAX.
// The vector's row is written whole first (zeros: also the columns of colliders the host pruned), then a
// hit ORs its node's bit into its collider's column: a read-modify-write of the lane's own row, and only on
// a hit.  Stores are one lane per vector, as in the rest of the family.
template <class Topo, int MODE, int TERMS>
__global__ void __launch_bounds__(256) k_evaluate_contacts(const ChainConsts<Topo::J> cc, const ContactsIO cio)
{
#pragma clang fp contract(off)
    constexpr int J = Topo::J;
    constexpr int D = Topo::D;
    static_assert(!Topo::kDH && (TERMS & kTermColliders) && J <= 32, "the Euler topologies' collider builds; a bit per node");
    using Acc = FitnessAcc<Topo, MODE, TERMS>;
    const int64_t DF = cc.dfree;
    const int64_t C = cio.columns;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < cio.n;
         n += (int64_t)gridDim.x * blockDim.x) {
        float x[D], pos[3 * J];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = dim_free(cc, d) ? cio.angles[n * DF + dim_rank(cc, d)] : cc.rest[d];
        // the forward pass (rest = x and a target nobody reads: the sums are dead)
        CandBuf<Topo, TERMS> cb;
        Acc acc(cc, nullptr, cc.aux + 4 * J, cb.v);
#pragma unroll
        for (int k = 1; k <= J; ++k) acc.node(cc, k, x + 3 * (k - 1), x + 3 * (k - 1), x + 3 * (k - 1), pos);
        if (cio.out_positions) {
#pragma unroll
            for (int d = 0; d < 3 * J; ++d) cio.out_positions[n * 3 * J + d] = pos[d];
        }
        uint32_t* const row = cio.out_contacts + n * C;
        for (int64_t c = 0; c < C; ++c) row[c] = 0u;
        // node k's decisions for the colliders first .. first + 31 into the row
        const auto report = [&](int k, int first, uint32_t hits) {
            while (hits != 0u) {
                const int c = first + __builtin_ctz(hits);
                hits &= hits - 1u;
                row[cio.column_of[c]] |= 1u << (k - 1);
            }
        };
        if constexpr (Acc::kDefer) {
            uint32_t m = acc.near_mask;
            while (m != 0u) {
                const int slot = __builtin_ctz(m);  // node slot + 1 = k
                const float* c = cb.v + 16 * slot;
                m &= m - 1u;
                const int k = slot + 1;
                for (int first = 0; first < cc.num_coll; first += kContactChunk) {
                    if constexpr (Acc::kCompactCand) {
                        constexpr int HW = kHwTrig<Topo, MODE, TERMS>;
                        const float a0 = c[0], a1 = c[1], a2 = c[2], b0 = c[3], b1 = c[4], b2 = c[5];
                        const float e0 = a1 * b2 - a2 * b1, e1 = a2 * b0 - a0 * b2, e2 = a0 * b1 - a1 * b0;
                        const float l = link_len<HW>(cc, k);
                        const float qx = c[6] - l * a0, qy = c[7] - l * a1, qz = c[8] - l * a2;
                        report(k, first,
                               node_contacts_obb(a0, b0, e0, a1, b1, e1, a2, b2, e2, c[6], c[7], c[8], qx, qy, qz,
                                                 cc.len[k], cc.coll, cc.coll_box, first, cc.num_coll));
                    } else if constexpr (kFastSat<Topo, MODE, TERMS>) {
                        report(k, first,
                               node_contacts_obb(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10],
                                                 c[11], c[12], c[13], c[14], c[15], cc.coll, cc.coll_box, first,
                                                 cc.num_coll));
                    } else {
                        report(k, first,
                               node_contacts(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11],
                                             c[12], c[13], c[14], c[15], cc.coll, first, cc.num_coll));
                    }
                }
            }
        } else {
#pragma unroll 1
            for (int k = 1; k <= J; ++k) {
                const int pk = cc.parent[k];
                const Frame& F = acc.F[k];
                const Frame& P = acc.F[pk];
                if (!near_collider(F.px, F.py, F.pz, P.px, P.py, P.pz, cc.coll_lim + (k - 1) * cc.num_coll, cc.coll,
                                   cc.num_coll IKPSO_CS_NONE))
                    continue;
                for (int first = 0; first < cc.num_coll; first += kContactChunk)
                    report(k, first,
                           node_contacts(F.r00, F.r01, F.r02, F.r10, F.r11, F.r12, F.r20, F.r21, F.r22, F.px, F.py,
                                         F.pz, P.px, P.py, P.pz, cc.len[k], cc.coll, first, cc.num_coll));
            }
        }
    }
}

// ikpso_solver_evaluate_contacts' evaluator kind (run_evaluate_kind): no compensation (the boxes are the
// solve's own, uncompensated), and no plain-term build.
struct EvalContacts {
    using IO = ContactsIO;
    static constexpr bool kPlainBuild = false;
    static int64_t n(const IO& io) { return io.n; }
    static float* frame_comp(IO&) { return nullptr; }
    static float* axis_y_comp(IO&) { return nullptr; }
    template <class Topo, int MODE, int TERMS>
    static constexpr auto kernel() { return &k_evaluate_contacts<Topo, MODE, TERMS>; }
};

}  // namespace ikpso
