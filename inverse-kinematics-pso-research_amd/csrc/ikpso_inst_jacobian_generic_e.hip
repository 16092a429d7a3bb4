// ikpso_inst_jacobian_generic_e.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of generic trees of 19-20 joints.
#define IKPSO_EVAL_KIND EvalJacobian
#include "ikpso_evallist_generic_e.h"
