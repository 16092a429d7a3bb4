// ikpso_inst_gradient_ref7.hip -- the gradient kernels (ikpso_solver_evaluate_gradient) of the reference scene.
#define IKPSO_EVAL_KIND EvalGradient
#include "ikpso_evallist_ref7.h"
