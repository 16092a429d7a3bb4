// ikpso_inst_contacts_generic_b.hip -- the contacts kernels (ikpso_solver_evaluate_contacts) of generic trees of 9-12 joints.
#define IKPSO_EVAL_KIND EvalContacts
#include "ikpso_evallist_generic_b.h"
