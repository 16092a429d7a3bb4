// ikpso_inst_evalframes_generic_d.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of generic trees of 17-18 joints.
#define IKPSO_EVAL_KIND EvalFrames
#include "ikpso_evallist_generic_d.h"
