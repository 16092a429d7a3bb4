// ikpso_inst_jacobian_generic_c.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of generic trees of 13-16 joints.
#define IKPSO_EVAL_KIND EvalJacobian
#include "ikpso_evallist_generic_c.h"
