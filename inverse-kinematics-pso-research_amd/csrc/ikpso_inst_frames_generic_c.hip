// ikpso_inst_frames_generic_c.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of generic trees of 13-16 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct FramesOps<TopoGeneric<13>>;
template struct FramesOps<TopoGeneric<14>>;
template struct FramesOps<TopoGeneric<15>>;
template struct FramesOps<TopoGeneric<16>>;
#endif
}  // namespace ikpso
