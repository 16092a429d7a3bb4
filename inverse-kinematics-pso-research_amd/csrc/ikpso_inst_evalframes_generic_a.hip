// ikpso_inst_evalframes_generic_a.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of generic trees of 1-8 joints.
#define IKPSO_EVAL_KIND EvalFrames
#include "ikpso_evallist_generic_a.h"
