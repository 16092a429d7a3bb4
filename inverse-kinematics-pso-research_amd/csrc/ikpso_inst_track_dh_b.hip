// ikpso_inst_track_dh_b.hip -- the resident track kernels (ikpso_solve_track) of folded serial chains (TopoDH) of 8-12 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TrackOps<TopoDH<8>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoDH<9>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoDH<10>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoDH<11>, IKPSO_ARITH_FAST>;
template struct TrackOps<TopoDH<12>, IKPSO_ARITH_FAST>;
#endif
}  // namespace ikpso
