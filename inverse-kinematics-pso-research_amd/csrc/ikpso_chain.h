// ikpso_chain.h -- the chain parser: a caller's node table and optional scene
// arrays to the ChainHost the kernels are dispatched on.  Pure host mathematics
// (ikpso_chain.cpp references nothing but libc and libm).
#pragma once

#include <vector>

#include "ikpso.h"
#include "ikpso_kernels.h"

namespace ikpso {

struct Extras {
    const float* positions = nullptr;  // host copy, [4J]
    float limit_weight = 0.0f;
    const float* soft_lo = nullptr;    // host copies, [D]
    const float* soft_hi = nullptr;
    const ikpso_collider* colliders = nullptr;  // host copy, [collider_count]
    int collider_count = 0;
    // IKPSO_FLAG_POSREF_NODE_SLOT: positions[] is [4*(J+2)] and node k's
    // reference position is read from slot k+1 (where FillPositions wrote it)
    bool posref_node_slot = false;
    const uint8_t* axis_mask = nullptr;  // host copy, [J + 1] (entry 0 ignored), or null
};

// The Euler form of the chain: topology, bounds, term flags and the aux block
// (reference positions, soft limits, the colliders within the arm's reach).
ikpso_status parse_chain(const std::vector<ikpso_node>& nodes, const ikpso_pso_config& pso,
                         const ikpso_fitness_config& fit, const Extras& ex, ChainHost& ch);

// The folded form (TopoDH) of a masked serial chain parse_chain accepted; false
// when it does not fold.
bool build_dh(const std::vector<ikpso_node>& nodes, const ChainHost& eu, const Extras& ex, ChainHost& dh);

// ikpso_solve_track_aim's axis in the folded chain's frame: a' = G a / |a| (G = ch.tip_rot), formed in
// fp64 and rounded once, so that R_eff a = W_J Rz(t_J) a'.  False, out untouched, for an axis that
// is not finite or shorter than 1e-6.
bool aim_axis_folded(const ChainHost& ch, const float axis[3], float out[3]);

}  // namespace ikpso
