// ikpso_inst_jacobian_serial_a.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of serial chains of 6, 7, 8 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct JacobianOps<TopoSerialTip<6>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoSerialTip<6>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoSerialTip<7>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoSerialTip<7>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoSerialTip<8>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoSerialTip<8>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
