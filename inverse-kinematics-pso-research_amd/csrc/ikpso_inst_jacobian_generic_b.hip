// ikpso_inst_jacobian_generic_b.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of generic trees of 9-12 joints.
#define IKPSO_EVAL_KIND EvalJacobian
#include "ikpso_evallist_generic_b.h"
