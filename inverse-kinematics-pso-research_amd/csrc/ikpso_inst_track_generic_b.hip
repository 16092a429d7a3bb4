// ikpso_inst_track_generic_b.hip -- the resident track kernels (ikpso_solve_track) of generic trees of 9-12 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct TrackOps<TopoGeneric<9>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<9>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<10>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<10>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<11>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<11>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<12>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<12>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
