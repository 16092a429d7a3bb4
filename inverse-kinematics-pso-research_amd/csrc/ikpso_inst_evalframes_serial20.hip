// ikpso_inst_evalframes_serial20.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of the 20-joint serial chain.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_SERIAL20
template struct EvalFramesOps<TopoSerialTip<20>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoSerialTip<20>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
