// ikpso_inst_evalframes_generic_b.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of generic trees of 9-12 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct EvalFramesOps<TopoGeneric<9>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<9>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<10>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<10>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<11>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<11>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<12>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<12>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
