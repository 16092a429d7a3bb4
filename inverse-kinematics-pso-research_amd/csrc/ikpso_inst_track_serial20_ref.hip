// ikpso_inst_track_serial20_ref.hip -- the resident track kernels (ikpso_solve_track) of the 20-joint serial chain.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_SERIAL20
template struct TrackOps<TopoSerialTip<20>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
