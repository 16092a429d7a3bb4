// ikpso_inst_gradient_generic_b.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of generic trees of 9-12 joints.
#define IKPSO_EVAL_KIND EvalGradient
#include "ikpso_evallist_generic_b.h"
