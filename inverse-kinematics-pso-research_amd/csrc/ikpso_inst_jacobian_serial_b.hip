// ikpso_inst_jacobian_serial_b.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of serial chains of 9, 10, 11 joints with a tip effector.
#define IKPSO_EVAL_KIND EvalJacobian
#include "ikpso_evallist_serial_b.h"
