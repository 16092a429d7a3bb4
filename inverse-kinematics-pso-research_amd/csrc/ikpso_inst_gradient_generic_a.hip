// ikpso_inst_gradient_generic_a.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of generic trees of 1-8 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct GradientOps<TopoGeneric<1>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<1>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<2>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<2>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<3>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<3>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<4>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<4>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<5>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<5>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<6>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<6>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<7>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<7>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<8>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<8>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
