// ikpso_inst_aim_dh_d.hip -- the aim track kernels (ikpso_solve_track_aim) of folded serial chains (TopoDH) of 10-11 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermAim, TopoDH<10>>;
template struct TermTrackOps<kTermAim, TopoDH<11>>;
#endif
}  // namespace ikpso
