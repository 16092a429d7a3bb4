// ikpso_evallist_serial_c.h -- the topologies of the evaluate family's serial_c units (serial chains of 12, 13, 14 joints with a tip effector):
// included by ikpso_inst_{evalframes,jacobian,gradient,contacts}_serial_c.hip after each defines IKPSO_EVAL_KIND.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
IKPSO_EVAL_INST(TopoSerialTip<12>)
IKPSO_EVAL_INST(TopoSerialTip<13>)
IKPSO_EVAL_INST(TopoSerialTip<14>)
#endif
}  // namespace ikpso
