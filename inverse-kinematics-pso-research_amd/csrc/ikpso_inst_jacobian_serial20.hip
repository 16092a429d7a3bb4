// ikpso_inst_jacobian_serial20.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of the 20-joint serial chain.
#define IKPSO_EVAL_KIND EvalJacobian
#include "ikpso_evallist_serial20.h"
