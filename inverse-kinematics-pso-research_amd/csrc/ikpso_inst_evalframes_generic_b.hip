// ikpso_inst_evalframes_generic_b.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of generic trees of 9-12 joints.
#define IKPSO_EVAL_KIND EvalFrames
#include "ikpso_evallist_generic_b.h"
