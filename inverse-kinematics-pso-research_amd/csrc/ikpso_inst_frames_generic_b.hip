// ikpso_inst_frames_generic_b.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of generic trees of 9-12 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct TermTrackOps<kTermOrient, TopoGeneric<9>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<10>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<11>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<12>>;
#endif
}  // namespace ikpso
