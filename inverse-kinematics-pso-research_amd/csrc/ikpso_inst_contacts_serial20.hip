// ikpso_inst_contacts_serial20.hip -- the contacts kernels (ikpso_solver_evaluate_contacts) of the 20-joint serial chain.
#define IKPSO_EVAL_KIND EvalContacts
#include "ikpso_evallist_serial20.h"
