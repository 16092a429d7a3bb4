// ikpso_inst_evalframes_serial_b.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of serial chains of 9, 10, 11 joints with a tip effector.
#define IKPSO_EVAL_KIND EvalFrames
#include "ikpso_evallist_serial_b.h"
