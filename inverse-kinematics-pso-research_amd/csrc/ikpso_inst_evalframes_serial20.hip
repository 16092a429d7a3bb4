// ikpso_inst_evalframes_serial20.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of the 20-joint serial chain.
#define IKPSO_EVAL_KIND EvalFrames
#include "ikpso_evallist_serial20.h"
