// ikpso_inst_contacts_generic_a.hip -- the contacts kernels (ikpso_solver_evaluate_contacts) of generic trees of 1-8 joints.
#define IKPSO_EVAL_KIND EvalContacts
#include "ikpso_evallist_generic_a.h"
