// ikpso_evallist_generic_e.h -- the topologies of the evaluate family's generic_e units (generic trees of 19-20 joints):
// included by ikpso_inst_{evalframes,jacobian,gradient,contacts}_generic_e.hip after each defines IKPSO_EVAL_KIND.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
IKPSO_EVAL_INST(TopoGeneric<19>)
IKPSO_EVAL_INST(TopoGeneric<20>)
#endif
}  // namespace ikpso
