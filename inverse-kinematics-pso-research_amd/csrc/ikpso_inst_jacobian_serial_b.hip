// ikpso_inst_jacobian_serial_b.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of serial chains of 9, 10, 11 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct JacobianOps<TopoSerialTip<9>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoSerialTip<9>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoSerialTip<10>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoSerialTip<10>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoSerialTip<11>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoSerialTip<11>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
