// ikpso_inst_frames_generic_a.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of generic trees of 1-8 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct TermTrackOps<kTermOrient, TopoGeneric<1>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<2>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<3>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<4>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<5>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<6>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<7>>;
template struct TermTrackOps<kTermOrient, TopoGeneric<8>>;
#endif
}  // namespace ikpso
