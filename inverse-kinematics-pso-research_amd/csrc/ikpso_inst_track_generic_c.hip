// ikpso_inst_track_generic_c.hip -- the resident track kernels (ikpso_solve_track) of generic trees of 13-15 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct TrackOps<TopoGeneric<13>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<13>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<14>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<14>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<15>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<15>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
