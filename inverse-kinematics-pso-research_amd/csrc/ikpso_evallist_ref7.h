// ikpso_evallist_ref7.h -- the topologies of the evaluate family's ref7 units (the reference scene):
// included by ikpso_inst_{evalframes,jacobian,gradient,contacts}_ref7.hip after each defines IKPSO_EVAL_KIND.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_REF7
IKPSO_EVAL_INST(TopoRef7)
#endif
}  // namespace ikpso
