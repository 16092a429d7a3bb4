// ikpso_topo_ops.h -- per-topology launch entry points.  The kernel templates
// (ikpso_resident.h, ikpso_stream.h, ikpso_evaluate.h) are instantiated per (topology, mode) in
// their own translation units (ikpso_inst_*.hip) so the build parallelises;
// the dispatcher (ikpso_kernels.hip) instantiates none of them: it calls these
// declarations, and reads the evaluator kinds' names from the kernels' headers.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "ikpso_device.h"
#include "ikpso_kernels.h"

namespace ikpso {

template <class Topo, int MODE>
struct ModeOps {
    static hipError_t resident(const ChainHost& ch, const SwarmIO& io, int block, hipStream_t stream);
    static hipError_t stream(const ChainHost& ch, const StreamIO& io, int iterations, hipStream_t stream);
    static hipError_t evaluate(const ChainHost& ch, const EvalIO& io, hipStream_t stream);
    static hipError_t coop(const ChainHost& ch, const SwarmIO& io, hipStream_t stream);
};

// The resident family's track kernels (ikpso_solve_track), apart from ModeOps so that their
// instantiations sit in translation units of their own (ikpso_inst_track_*.hip).
template <class Topo, int MODE>
struct TrackOps {
    static hipError_t resident(const ChainHost& ch, const SwarmIO& io, int block, hipStream_t stream);
};

// The track kernels with a term of their own (FAST only), in units of their own again:
//   TermTrackOps<kTermOrient, TopoDH<J>>    ikpso_solve_track_pose    ikpso_inst_pose_dh_*.hip
//   TermTrackOps<kTermAim, TopoDH<J>>       ikpso_solve_track_aim     ikpso_inst_aim_dh_*.hip
//   TermTrackOps<kTermOrient, Euler Topo>   ikpso_solve_track_frames  ikpso_inst_frames_*.hip
template <int TERM, class Topo>
struct TermTrackOps {
    static hipError_t track(const ChainHost& ch, const SwarmIO& io, int block, hipStream_t stream);
};

// The evaluate kernels with units of their own (every Euler topology, both modes), likewise.  Kind
// (ikpso_evaluate.h; ikpso_jacobian.h, ikpso_gradient.h, ikpso_contacts.h) names the parameter block and the kernel:
//   EvalOps<EvalFrames, ...>     ikpso_solver_evaluate_frames    ikpso_inst_evalframes_*.hip
//   EvalOps<EvalJacobian, ...>   ikpso_solver_evaluate_jacobian  ikpso_inst_jacobian_*.hip
//   EvalOps<EvalGradient, ...>   ikpso_solver_evaluate_gradient  ikpso_inst_gradient_*.hip
//   EvalOps<EvalContacts, ...>   ikpso_solver_evaluate_contacts  ikpso_inst_contacts_*.hip
template <class Kind, class Topo, int MODE>
struct EvalOps {
    static hipError_t evaluate(const ChainHost& ch, const typename Kind::IO& io, hipStream_t stream);
};

// The folded chain (TopoDH) has FAST kernels only: REFERENCE runs of such a
// chain use its Euler form.
template <class Topo>
struct TopoOps {
    static constexpr bool kRef = !Topo::kDH;
    // f(mode as a compile-time constant) for the arithmetic mode `mode`
    template <class F>
    static hipError_t with_mode(int mode, F&& f)
    {
        if (mode == IKPSO_ARITH_REFERENCE) {
            if constexpr (kRef) return f(std::integral_constant<int, IKPSO_ARITH_REFERENCE>{});
            return hipErrorNotSupported;
        }
        return f(std::integral_constant<int, IKPSO_ARITH_FAST>{});
    }
    static hipError_t resident(const ChainHost& ch, int mode, const SwarmIO& io, int block, hipStream_t s)
    {
        return with_mode(mode, [&](auto m) { return ModeOps<Topo, decltype(m)::value>::resident(ch, io, block, s); });
    }
    static hipError_t track(const ChainHost& ch, int mode, const SwarmIO& io, int block, hipStream_t s)
    {
        return with_mode(mode, [&](auto m) { return TrackOps<Topo, decltype(m)::value>::resident(ch, io, block, s); });
    }
    // TERM's track kernels: the folded chain has the tip's orientation and aim terms, the Euler topologies
    // the orientation term per effector; no other kernel has either
    template <int TERM>
    static hipError_t term_track(const ChainHost& ch, int mode, const SwarmIO& io, int block, hipStream_t s)
    {
        if constexpr (TERM == kTermOrient || (TERM == kTermAim && Topo::kDH)) {
            if (mode == IKPSO_ARITH_FAST) return TermTrackOps<TERM, Topo>::track(ch, io, block, s);
        }
        return hipErrorNotSupported;
    }
    static hipError_t stream(const ChainHost& ch, int mode, const StreamIO& io, int iterations, hipStream_t s)
    {
        return with_mode(mode, [&](auto m) { return ModeOps<Topo, decltype(m)::value>::stream(ch, io, iterations, s); });
    }
    static hipError_t evaluate(const ChainHost& ch, int mode, const EvalIO& io, hipStream_t s)
    {
        return with_mode(mode, [&](auto m) { return ModeOps<Topo, decltype(m)::value>::evaluate(ch, io, s); });
    }
    template <class Kind>
    static hipError_t evaluate_kind(const ChainHost& ch, int mode, const typename Kind::IO& io, hipStream_t s)
    {
        if constexpr (Topo::kDH)
            return hipErrorNotSupported;  // the solver evaluates through its Euler chain (run_evaluate)
        else
            return with_mode(mode, [&](auto m) { return EvalOps<Kind, Topo, decltype(m)::value>::evaluate(ch, io, s); });
    }
    static hipError_t coop(const ChainHost& ch, int mode, const SwarmIO& io, hipStream_t s)
    {
        return with_mode(mode, [&](auto m) { return ModeOps<Topo, decltype(m)::value>::coop(ch, io, s); });
    }
};

}  // namespace ikpso
