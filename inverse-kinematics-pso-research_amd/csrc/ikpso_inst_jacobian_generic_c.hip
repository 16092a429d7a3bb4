// ikpso_inst_jacobian_generic_c.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of generic trees of 13-16 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct JacobianOps<TopoGeneric<13>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<13>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<14>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<14>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<15>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<15>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<16>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<16>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
