// ikpso_inst_contacts_generic_c.hip -- the contacts kernels (ikpso_solver_evaluate_contacts) of generic trees of 13-16 joints.
#define IKPSO_EVAL_KIND EvalContacts
#include "ikpso_evallist_generic_c.h"
