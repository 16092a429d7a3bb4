// ikpso_inst_gradient_serial_c.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of serial chains of 12, 13, 14 joints with a tip effector.
#define IKPSO_EVAL_KIND EvalGradient
#include "ikpso_evallist_serial_c.h"
