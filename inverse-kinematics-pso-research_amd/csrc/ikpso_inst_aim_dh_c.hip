// ikpso_inst_aim_dh_c.hip -- the aim track kernels (ikpso_solve_track_aim) of folded serial chains (TopoDH) of 8-9 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermAim, TopoDH<8>>;
template struct TermTrackOps<kTermAim, TopoDH<9>>;
#endif
}  // namespace ikpso
