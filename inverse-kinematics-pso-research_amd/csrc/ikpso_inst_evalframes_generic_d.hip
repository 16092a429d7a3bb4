// ikpso_inst_evalframes_generic_d.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of generic trees of 17-18 joints.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
template struct EvalFramesOps<TopoGeneric<17>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<17>, IKPSO_ARITH_REFERENCE>;
template struct EvalFramesOps<TopoGeneric<18>, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoGeneric<18>, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
