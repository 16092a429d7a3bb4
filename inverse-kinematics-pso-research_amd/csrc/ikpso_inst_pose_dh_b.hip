// ikpso_inst_pose_dh_b.hip -- the pose track kernels (ikpso_solve_track_pose) of folded serial chains (TopoDH) of 6-7 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermOrient, TopoDH<6>>;
template struct TermTrackOps<kTermOrient, TopoDH<7>>;
#endif
}  // namespace ikpso
