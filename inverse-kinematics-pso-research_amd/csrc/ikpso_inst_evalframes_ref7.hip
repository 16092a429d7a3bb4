// ikpso_inst_evalframes_ref7.hip -- the evaluate kernels with node rotations (ikpso_solver_evaluate_frames) of the reference scene.
#define IKPSO_EVAL_KIND EvalFrames
#include "ikpso_evallist_ref7.h"
