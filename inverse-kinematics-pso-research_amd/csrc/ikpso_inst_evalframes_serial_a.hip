// ikpso_inst_evalframes_serial_a.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of serial chains of 6, 7, 8 joints with a tip effector.
#define IKPSO_EVAL_KIND EvalFrames
#include "ikpso_evallist_serial_a.h"
