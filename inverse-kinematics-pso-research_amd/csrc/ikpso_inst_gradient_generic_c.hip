// ikpso_inst_gradient_generic_c.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of generic trees of 13-16 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct GradientOps<TopoGeneric<13>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<13>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<14>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<14>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<15>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<15>, IKPSO_ARITH_REFERENCE>;
template struct GradientOps<TopoGeneric<16>, IKPSO_ARITH_FAST>;
template struct GradientOps<TopoGeneric<16>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
