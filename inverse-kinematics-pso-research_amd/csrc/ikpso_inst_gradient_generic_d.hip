// ikpso_inst_gradient_generic_d.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of generic trees of 17-18 joints.
#define IKPSO_EVAL_KIND EvalGradient
#include "ikpso_evallist_generic_d.h"
