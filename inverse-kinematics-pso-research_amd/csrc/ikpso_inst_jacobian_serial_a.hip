// ikpso_inst_jacobian_serial_a.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of serial chains of 6, 7, 8 joints with a tip effector.
#define IKPSO_EVAL_KIND EvalJacobian
#include "ikpso_evallist_serial_a.h"
