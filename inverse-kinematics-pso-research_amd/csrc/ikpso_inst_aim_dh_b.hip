// ikpso_inst_aim_dh_b.hip -- the aim track kernels (ikpso_solve_track_aim) of folded serial chains (TopoDH) of 6-7 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermAim, TopoDH<6>>;
template struct TermTrackOps<kTermAim, TopoDH<7>>;
#endif
}  // namespace ikpso
