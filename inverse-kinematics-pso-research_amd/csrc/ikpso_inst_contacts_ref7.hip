// ikpso_inst_contacts_ref7.hip -- the contacts kernels (ikpso_solver_evaluate_contacts) of the reference scene.
#define IKPSO_EVAL_KIND EvalContacts
#include "ikpso_evallist_ref7.h"
