// ikpso_inst_frames_serial_a.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of serial chains of 6, 7, 8 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermOrient, TopoSerialTip<6>>;
template struct TermTrackOps<kTermOrient, TopoSerialTip<7>>;
template struct TermTrackOps<kTermOrient, TopoSerialTip<8>>;
#endif
}  // namespace ikpso
