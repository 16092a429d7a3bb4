// ikpso_inst_frames_generic_e.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of generic trees of 19-20 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct TermTrackOps<kTermOrient, TopoGeneric<19>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<20>>;
#endif
}  // namespace ikpso
