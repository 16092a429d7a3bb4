// ikpso_inst_frames_generic_a.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of generic trees of 1-8 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct FramesOps<TopoGeneric<1>>;
template struct FramesOps<TopoGeneric<2>>;
template struct FramesOps<TopoGeneric<3>>;
template struct FramesOps<TopoGeneric<4>>;
template struct FramesOps<TopoGeneric<5>>;
template struct FramesOps<TopoGeneric<6>>;
template struct FramesOps<TopoGeneric<7>>;
template struct FramesOps<TopoGeneric<8>>;
#endif
}  // namespace ikpso
