// ikpso_inst_gradient_serial_b.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of serial chains of 9, 10, 11 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct GradientOps<TopoSerialTip<9>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoSerialTip<9>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoSerialTip<10>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoSerialTip<10>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoSerialTip<11>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoSerialTip<11>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
