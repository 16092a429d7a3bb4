// ikpso_evallist_generic_a.h -- the topologies of the evaluate family's generic_a units (generic trees of 1-8 joints):
// included by ikpso_inst_{evalframes,jacobian,gradient,contacts}_generic_a.hip after each defines IKPSO_EVAL_KIND.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_OTHERS
IKPSO_EVAL_INST(TopoGeneric<1>)
IKPSO_EVAL_INST(TopoGeneric<2>)
IKPSO_EVAL_INST(TopoGeneric<3>)
IKPSO_EVAL_INST(TopoGeneric<4>)
IKPSO_EVAL_INST(TopoGeneric<5>)
IKPSO_EVAL_INST(TopoGeneric<6>)
IKPSO_EVAL_INST(TopoGeneric<7>)
IKPSO_EVAL_INST(TopoGeneric<8>)
#endif
}  // namespace ikpso
