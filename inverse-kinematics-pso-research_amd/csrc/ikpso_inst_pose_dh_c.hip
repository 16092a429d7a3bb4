// ikpso_inst_pose_dh_c.hip -- the pose track kernels (ikpso_solve_track_pose) of folded serial chains (TopoDH) of 8-9 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermOrient, TopoDH<8>>;
template struct TermTrackOps<kTermOrient, TopoDH<9>>;
#endif
}  // namespace ikpso
