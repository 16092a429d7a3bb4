// ikpso_inst_gradient_serial_a.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of serial chains of 6, 7, 8 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct GradientOps<TopoSerialTip<6>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoSerialTip<6>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoSerialTip<7>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoSerialTip<7>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoSerialTip<8>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoSerialTip<8>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
