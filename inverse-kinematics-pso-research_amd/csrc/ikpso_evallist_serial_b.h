// ikpso_evallist_serial_b.h -- the topologies of the evaluate family's serial_b units (serial chains of 9, 10, 11 joints with a tip effector):
// included by ikpso_inst_{evalframes,jacobian,gradient,contacts}_serial_b.hip after each defines IKPSO_EVAL_KIND.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
IKPSO_EVAL_INST(TopoSerialTip<9>)
IKPSO_EVAL_INST(TopoSerialTip<10>)
IKPSO_EVAL_INST(TopoSerialTip<11>)
#endif
}  // namespace ikpso
