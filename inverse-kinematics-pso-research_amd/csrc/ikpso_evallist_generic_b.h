// ikpso_evallist_generic_b.h -- the topologies of the evaluate family's generic_b units (generic trees of 9-12 joints):
// included by ikpso_inst_{evalframes,jacobian,gradient,contacts}_generic_b.hip after each defines IKPSO_EVAL_KIND.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
IKPSO_EVAL_INST(TopoGeneric<9>)
IKPSO_EVAL_INST(TopoGeneric<10>)
IKPSO_EVAL_INST(TopoGeneric<11>)
IKPSO_EVAL_INST(TopoGeneric<12>)
#endif
}  // namespace ikpso
