// ikpso_evallist_generic_d.h -- the topologies of the evaluate family's generic_d units (generic trees of 17-18 joints):
// included by ikpso_inst_{evalframes,jacobian,gradient,contacts}_generic_d.hip after each defines IKPSO_EVAL_KIND.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
IKPSO_EVAL_INST(TopoGeneric<17>)
IKPSO_EVAL_INST(TopoGeneric<18>)
#endif
}  // namespace ikpso
