// ikpso_inst_gradient_serial20.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of the 20-joint serial chain.
#define IKPSO_EVAL_KIND EvalGradient
#include "ikpso_evallist_serial20.h"
