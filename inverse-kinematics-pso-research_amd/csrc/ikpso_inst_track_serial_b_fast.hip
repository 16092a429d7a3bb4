// ikpso_inst_track_serial_b_fast.hip -- the resident track kernels (ikpso_solve_track) of serial chains of 9, 10, 11 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TrackOps<TopoSerialTip<9>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoSerialTip<10>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoSerialTip<11>, IKPSO_ARITH_FAST>;
#endif
}  // namespace ikpso
