// ikpso_inst_evalframes_generic_a.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of generic trees of 1-8 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct EvalFramesOps<TopoGeneric<1>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<1>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<2>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<2>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<3>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<3>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<4>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<4>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<5>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<5>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<6>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<6>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<7>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<7>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<8>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<8>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
