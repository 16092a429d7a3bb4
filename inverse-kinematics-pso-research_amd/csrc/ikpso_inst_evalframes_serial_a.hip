// ikpso_inst_evalframes_serial_a.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of serial chains of 6, 7, 8 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct EvalFramesOps<TopoSerialTip<6>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoSerialTip<6>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoSerialTip<7>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoSerialTip<7>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoSerialTip<8>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoSerialTip<8>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
