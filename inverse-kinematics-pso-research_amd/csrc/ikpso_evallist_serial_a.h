// ikpso_evallist_serial_a.h -- the topologies of the evaluate family's serial_a units (serial chains of 6, 7, 8 joints with a tip effector):
// included by ikpso_inst_{evalframes,jacobian,gradient,contacts}_serial_a.hip after each defines IKPSO_EVAL_KIND.
#include "ikpso_topo_impl.h"

namespace ikpso {
#if IKPSO_WITH_DH
IKPSO_EVAL_INST(TopoSerialTip<6>)
IKPSO_EVAL_INST(TopoSerialTip<7>)
IKPSO_EVAL_INST(TopoSerialTip<8>)
#endif
}  // namespace ikpso
