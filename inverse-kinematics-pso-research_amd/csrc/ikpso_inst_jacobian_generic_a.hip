// ikpso_inst_jacobian_generic_a.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of generic trees of 1-8 joints.
#define IKPSO_EVAL_KIND EvalJacobian
#include "ikpso_evallist_generic_a.h"
