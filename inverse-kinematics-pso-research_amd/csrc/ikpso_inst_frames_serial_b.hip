// ikpso_inst_frames_serial_b.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of serial chains of 9, 10, 11 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermOrient, TopoSerialTip<9>>;
template struct TermTrackOps<kTermOrient, TopoSerialTip<10>>;
template struct TermTrackOps<kTermOrient, TopoSerialTip<11>>;
#endif
}  // namespace ikpso
