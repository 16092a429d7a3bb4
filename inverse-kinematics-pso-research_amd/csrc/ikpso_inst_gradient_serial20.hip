// ikpso_inst_gradient_serial20.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of the 20-joint serial chain.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_SERIAL20
template struct GradientOps<TopoSerialTip<20>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoSerialTip<20>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
