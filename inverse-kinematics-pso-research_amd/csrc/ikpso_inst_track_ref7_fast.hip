// ikpso_inst_track_ref7_fast.hip -- the resident track kernels (ikpso_solve_track) of the reference scene.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_REF7
template struct TrackOps<TopoRef7, IKPSO_ARITH_FAST>;
#endif
}  // namespace ikpso
