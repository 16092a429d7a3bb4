// ikpso_inst_track_generic_a.hip -- the resident track kernels (ikpso_solve_track) of generic trees of 1-8 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct TrackOps<TopoGeneric<1>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<1>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<2>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<2>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<3>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<3>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<4>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<4>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<5>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<5>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<6>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<6>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<7>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<7>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<8>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<8>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
