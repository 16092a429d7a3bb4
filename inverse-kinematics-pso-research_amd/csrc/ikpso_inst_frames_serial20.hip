// ikpso_inst_frames_serial20.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of the 20-joint serial chain.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_SERIAL20
template struct TermTrackOps<kTermOrient, TopoSerialTip<20>>;
#endif
}  // namespace ikpso
