// ikpso_inst_track_dh_a.hip -- the resident track kernels (ikpso_solve_track) of folded serial chains (TopoDH) of 3-7 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TrackOps<TopoDH<3>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoDH<4>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoDH<5>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoDH<6>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoDH<7>, IKPSO_ARITH_FAST>;
#endif
}  // namespace ikpso
