// ikpso_inst_track_generic_d.hip -- the resident track kernels (ikpso_solve_track) of generic trees of 16-18 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct TrackOps<TopoGeneric<16>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<16>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<17>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<17>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoGeneric<18>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoGeneric<18>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
