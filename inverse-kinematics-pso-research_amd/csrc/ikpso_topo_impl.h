// ikpso_topo_impl.h -- definitions of ModeOps<Topo, MODE>, TrackOps<Topo, MODE>, TermTrackOps<TERM, Topo>
// and EvalOps<Kind, Topo, MODE>; include from the ikpso_inst_*.hip translation units, followed by explicit
// instantiations.
#pragma once

#include "ikpso_contacts.h"
#include "ikpso_coop.h"
#include "ikpso_evaluate.h"
#include "ikpso_gradient.h"
#include "ikpso_jacobian.h"
#include "ikpso_resident.h"
#include "ikpso_stream.h"
#include "ikpso_topo_ops.h"

namespace ikpso {

template <class Topo, int MODE>
hipError_t ModeOps<Topo, MODE>::resident(const ChainHost& ch, const SwarmIO& io, int block, hipStream_t s)
{
    return run_resident<Topo, MODE>(ch, io, block, s);
}

template <class Topo, int MODE>
hipError_t TrackOps<Topo, MODE>::resident(const ChainHost& ch, const SwarmIO& io, int block, hipStream_t s)
{
    return run_resident<Topo, MODE, true>(ch, io, block, s);
}

template <int TERM, class Topo>
hipError_t TermTrackOps<TERM, Topo>::track(const ChainHost& ch, const SwarmIO& io, int block, hipStream_t s)
{
    return run_resident_term<Topo, TERM>(ch, io, block, s);
}

template <class Topo, int MODE>
hipError_t ModeOps<Topo, MODE>::stream(const ChainHost& ch, const StreamIO& io, int iterations, hipStream_t s)
{
    return run_stream_terms<Topo, MODE>(ch, io, iterations, s);
}

template <class Topo, int MODE>
hipError_t ModeOps<Topo, MODE>::evaluate(const ChainHost& ch, const EvalIO& io, hipStream_t s)
{
    return run_evaluate<Topo, MODE>(ch, io, s);
}

template <class Kind, class Topo, int MODE>
hipError_t EvalOps<Kind, Topo, MODE>::evaluate(const ChainHost& ch, const typename Kind::IO& io, hipStream_t s)
{
    return run_evaluate_kind<Kind, Topo, MODE>(ch, io, s);
}

// A unit's evaluate kernels of one topology, both arithmetic modes (the ikpso_evallist_*.h lists; the unit
// defines IKPSO_EVAL_KIND).
#define IKPSO_EVAL_INST(...)                                                      \
    template struct EvalOps<IKPSO_EVAL_KIND, __VA_ARGS__, IKPSO_ARITH_FAST>; \
    template struct EvalOps<IKPSO_EVAL_KIND, __VA_ARGS__, IKPSO_ARITH_REFERENCE>;

template <class Topo, int MODE>
hipError_t ModeOps<Topo, MODE>::coop(const ChainHost& ch, const SwarmIO& io, hipStream_t s)
{
    if constexpr (Topo::kGeneric)
        return hipErrorNotSupported;  // generic trees take the streaming kernels
    else
        return run_coop<Topo, MODE>(ch, io, s);
}

}  // namespace ikpso
