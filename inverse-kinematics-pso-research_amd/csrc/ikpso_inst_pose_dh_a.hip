// ikpso_inst_pose_dh_a.hip -- the pose track kernels (ikpso_solve_track_pose) of folded serial chains (TopoDH) of 3-5 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermOrient, TopoDH<3>>;
template struct TermTrackOps<kTermOrient, TopoDH<4>>;
template struct TermTrackOps<kTermOrient, TopoDH<5>>;
#endif
}  // namespace ikpso
