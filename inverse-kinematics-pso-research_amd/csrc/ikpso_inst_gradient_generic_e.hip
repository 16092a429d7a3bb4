// ikpso_inst_gradient_generic_e.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of generic trees of 19-20 joints.
#define IKPSO_EVAL_KIND EvalGradient
#include "ikpso_evallist_generic_e.h"
