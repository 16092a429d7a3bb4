// ikpso_evallist_generic_c.h -- the topologies of the evaluate family's generic_c units (generic trees of 13-16 joints):
// included by ikpso_inst_{evalframes,jacobian,gradient,contacts}_generic_c.hip after each defines IKPSO_EVAL_KIND.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
IKPSO_EVAL_INST(TopoGeneric<13>)
IKPSO_EVAL_INST(TopoGeneric<14>)
IKPSO_EVAL_INST(TopoGeneric<15>)
IKPSO_EVAL_INST(TopoGeneric<16>)
#endif
}  // namespace ikpso
