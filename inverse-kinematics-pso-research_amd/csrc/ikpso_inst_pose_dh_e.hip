// ikpso_inst_pose_dh_e.hip -- the pose track kernels (ikpso_solve_track_pose) of folded serial chains (TopoDH) of 12 free angles.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermOrient, TopoDH<12>>;
#endif
}  // namespace ikpso
