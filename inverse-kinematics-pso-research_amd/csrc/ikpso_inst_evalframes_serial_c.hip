// ikpso_inst_evalframes_serial_c.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of serial chains of 12, 13, 14 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct EvalFramesOps<TopoSerialTip<12>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoSerialTip<12>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoSerialTip<13>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoSerialTip<13>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoSerialTip<14>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoSerialTip<14>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
