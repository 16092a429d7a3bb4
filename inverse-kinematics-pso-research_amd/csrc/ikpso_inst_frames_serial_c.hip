// ikpso_inst_frames_serial_c.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of serial chains of 12, 13, 14 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct TermTrackOps<kTermOrient, TopoSerialTip<12>>;
template struct TermTrackOps<kTermOrient, TopoSerialTip<13>>;
template struct TermTrackOps<kTermOrient, TopoSerialTip<14>>;
#endif
}  // namespace ikpso
