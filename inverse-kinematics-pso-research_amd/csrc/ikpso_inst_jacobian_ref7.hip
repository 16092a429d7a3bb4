// ikpso_inst_jacobian_ref7.hip -- the Jacobian kernels (ikpso_solver_evaluate_jacobian) of the reference scene.
#define IKPSO_EVAL_KIND EvalJacobian
#include "ikpso_evallist_ref7.h"
