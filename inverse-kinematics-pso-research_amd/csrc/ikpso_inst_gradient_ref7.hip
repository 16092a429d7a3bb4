// ikpso_inst_gradient_ref7.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of the reference scene.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_REF7
template struct GradientOps<TopoRef7, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoRef7, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
