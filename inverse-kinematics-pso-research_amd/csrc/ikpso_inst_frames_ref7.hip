// ikpso_inst_frames_ref7.hip -- the effector-frame track kernels (ikpso_solve_track_frames) of the reference scene.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_REF7
template struct TermTrackOps<kTermOrient, TopoRef7>;
#endif
}  // namespace ikpso
