// ikpso_inst_track_generic_e.hip -- the resident track kernels (ikpso_solve_track) of generic trees of 19-20 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct TrackOps<TopoGeneric<19>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<19>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<20>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<20>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
