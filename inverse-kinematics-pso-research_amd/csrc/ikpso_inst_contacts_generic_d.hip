// ikpso_inst_contacts_generic_d.hip -- the contacts kernels (ikpso_solver_evaluate_contacts) of generic trees of 17-18 joints.
#define IKPSO_EVAL_KIND EvalContacts
#include "ikpso_evallist_generic_d.h"
