// ikpso_inst_jacobian_generic_d.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of generic trees of 17-18 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct JacobianOps<TopoGeneric<17>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<17>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<18>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<18>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
