// ikpso_inst_gradient_generic_e.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of generic trees of 19-20 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct GradientOps<TopoGeneric<19>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<19>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<20>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<20>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
