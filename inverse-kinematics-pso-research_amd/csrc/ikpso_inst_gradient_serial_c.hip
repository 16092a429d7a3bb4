// ikpso_inst_gradient_serial_c.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of serial chains of 12, 13, 14 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct GradientOps<TopoSerialTip<12>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoSerialTip<12>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoSerialTip<13>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoSerialTip<13>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoSerialTip<14>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoSerialTip<14>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
