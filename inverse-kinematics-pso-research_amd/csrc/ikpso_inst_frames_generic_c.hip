// ikpso_inst_frames_generic_c.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of generic trees of 13-16 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct TermTrackOps<kTermOrient, TopoGeneric<13>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<14>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<15>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<16>>;
#endif
}  // namespace ikpso
