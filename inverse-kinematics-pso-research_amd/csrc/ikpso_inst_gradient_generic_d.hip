// ikpso_inst_gradient_generic_d.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of generic trees of 17-18 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct GradientOps<TopoGeneric<17>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<17>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<18>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<18>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
