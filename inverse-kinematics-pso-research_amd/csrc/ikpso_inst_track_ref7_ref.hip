// ikpso_inst_track_ref7_ref.hip -- the resident track kernels (ikpso_solve_track) of the reference scene.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_REF7
template struct TrackOps<TopoRef7, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
