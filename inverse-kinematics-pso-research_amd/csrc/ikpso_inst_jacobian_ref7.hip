// ikpso_inst_jacobian_ref7.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of the reference scene.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_REF7
template struct JacobianOps<TopoRef7, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoRef7, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
