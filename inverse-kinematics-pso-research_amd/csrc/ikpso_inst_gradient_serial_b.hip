// ikpso_inst_gradient_serial_b.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of serial chains of 9, 10, 11 joints with a tip effector.
#define IKPSO_EVAL_KIND EvalGradient
#include "ikpso_evallist_serial_b.h"
