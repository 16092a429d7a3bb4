// ikpso_inst_evalframes_ref7.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of the reference scene.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_REF7
template struct EvalFramesOps<TopoRef7, IKPSO_ARITH_FAST>;
template struct EvalFramesOps<TopoRef7, IKPSO_ARITH_REFERENCE>;
#endif
}  // namespace ikpso
