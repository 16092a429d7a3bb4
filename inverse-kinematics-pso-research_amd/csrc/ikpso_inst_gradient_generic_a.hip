// ikpso_inst_gradient_generic_a.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of generic trees of 1-8 joints.
#define IKPSO_EVAL_KIND EvalGradient
#include "ikpso_evallist_generic_a.h"
