// ikpso_inst_evalframes_generic_c.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of generic trees of 13-16 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct EvalFramesOps<TopoGeneric<13>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<13>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<14>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<14>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<15>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<15>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<16>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<16>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
