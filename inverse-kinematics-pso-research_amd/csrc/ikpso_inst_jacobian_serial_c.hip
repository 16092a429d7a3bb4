// ikpso_inst_jacobian_serial_c.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of serial chains of 12, 13, 14 joints with a tip effector.
#define IKPSO_EVAL_KIND EvalJacobian
#include "ikpso_evallist_serial_c.h"
