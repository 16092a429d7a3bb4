// ikpso_inst_jacobian_generic_b.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of generic trees of 9-12 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct JacobianOps<TopoGeneric<9>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<9>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<10>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<10>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<11>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<11>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<12>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<12>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
