// ikpso_inst_pose_dh_d.hip -- the pose track kernels (ikpso_solve_track_pose) of folded serial chains (TopoDH) of 10-11 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermOrient, TopoDH<10>>;
template struct TermTrackOps<kTermOrient, TopoDH<11>>;
#endif
}  // namespace ikpso
