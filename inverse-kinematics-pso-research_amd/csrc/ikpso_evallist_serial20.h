// ikpso_evallist_serial20.h -- the topologies of the evaluate family's serial20 units (the 20-joint serial chain):
// included by ikpso_inst_{evalframes,jacobian,gradient,contacts}_serial20.hip after each defines IKPSO_EVAL_KIND.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_SERIAL20
IKPSO_EVAL_INST(TopoSerialTip<20>)
#endif
}  // namespace ikpso
