// ikpso_inst_frames_generic_d.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of generic trees of 17-18 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct TermTrackOps<kTermOrient, TopoGeneric<17>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<18>>;
#endif
}  // namespace ikpso
