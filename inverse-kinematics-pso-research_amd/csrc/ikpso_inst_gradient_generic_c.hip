// ikpso_inst_gradient_generic_c.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of generic trees of 13-16 joints.
#define IKPSO_EVAL_KIND EvalGradient
#include "ikpso_evallist_generic_c.h"
