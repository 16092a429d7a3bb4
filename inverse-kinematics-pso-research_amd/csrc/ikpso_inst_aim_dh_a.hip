// ikpso_inst_aim_dh_a.hip -- the aim track kernels (ikpso_solve_track_aim) of folded serial chains (TopoDH) of 3-5 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermAim, TopoDH<3>>;
template struct TermTrackOps<kTermAim, TopoDH<4>>;
template struct TermTrackOps<kTermAim, TopoDH<5>>;
#endif
}  // namespace ikpso
