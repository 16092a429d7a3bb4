// ikpso_inst_aim_dh_e.hip -- the aim track kernels (ikpso_solve_track_aim) of folded serial chains (TopoDH) of 12 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermAim, TopoDH<12>>;
#endif
}  // namespace ikpso
