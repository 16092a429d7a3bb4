// ikpso_inst_gradient_serial_a.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of serial chains of 6, 7, 8 joints with a tip effector.
#define IKPSO_EVAL_KIND EvalGradient
#include "ikpso_evallist_serial_a.h"
