// ikpso_inst_track_serial_c_fast.hip -- the resident track kernels (ikpso_solve_track) of serial chains of 12, 13, 14 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TrackOps<TopoSerialTip<12>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoSerialTip<13>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoSerialTip<14>, IKPSO_ARITH_FAST>;
#endif
}  // namespace ikpso
