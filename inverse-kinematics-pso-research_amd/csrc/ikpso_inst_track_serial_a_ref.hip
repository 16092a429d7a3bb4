// ikpso_inst_track_serial_a_ref.hip -- the resident track kernels (ikpso_solve_track) of serial chains of 6, 7, 8 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TrackOps<TopoSerialTip<6>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoSerialTip<7>, IKPSO_ARITH_REFERENCE>;
template struct TrackOps<TopoSerialTip<8>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
