// ikpso_inst_jacobian_serial_c.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of serial chains of 12, 13, 14 joints with a tip effector.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
template struct JacobianOps<TopoSerialTip<12>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoSerialTip<12>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoSerialTip<13>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoSerialTip<13>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoSerialTip<14>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoSerialTip<14>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
