// ikpso_inst_gradient_generic_b.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of generic trees of 9-12 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct GradientOps<TopoGeneric<9>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<9>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<10>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<10>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<11>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<11>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<12>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<12>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
