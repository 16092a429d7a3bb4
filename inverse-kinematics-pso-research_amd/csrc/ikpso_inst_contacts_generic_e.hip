// ikpso_inst_contacts_generic_e.hip -- the contacts kernels (ikpso_solver_evaluate_contacts) of generic trees of 19-20 joints.
#define IKPSO_EVAL_KIND EvalContacts
#include "ikpso_evallist_generic_e.h"
