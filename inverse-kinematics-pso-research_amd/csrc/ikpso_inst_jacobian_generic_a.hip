// ikpso_inst_jacobian_generic_a.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of generic trees of 1-8 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct JacobianOps<TopoGeneric<1>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<1>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<2>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<2>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<3>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<3>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<4>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<4>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<5>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<5>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<6>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<6>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<7>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<7>, IKPSO_ARITH_REFERENCE>;
template struct JacobianOps<TopoGeneric<8>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoGeneric<8>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
