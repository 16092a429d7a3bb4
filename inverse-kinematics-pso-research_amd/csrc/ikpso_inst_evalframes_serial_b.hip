// ikpso_inst_evalframes_serial_b.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of serial chains of 9, 10, 11 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct EvalFramesOps<TopoSerialTip<9>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoSerialTip<9>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoSerialTip<10>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoSerialTip<10>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoSerialTip<11>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoSerialTip<11>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
