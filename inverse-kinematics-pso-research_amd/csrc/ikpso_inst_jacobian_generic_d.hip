// ikpso_inst_jacobian_generic_d.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of generic trees of 17-18 joints.
#define IKPSO_EVAL_KIND EvalJacobian
#include "ikpso_evallist_generic_d.h"
