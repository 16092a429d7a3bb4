// ikpso_inst_jacobian_serial20.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of the 20-joint serial chain.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_SERIAL20
template struct JacobianOps<TopoSerialTip<20>, IKPSO_ARITH_FAST>;
template struct JacobianOps<TopoSerialTip<20>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
