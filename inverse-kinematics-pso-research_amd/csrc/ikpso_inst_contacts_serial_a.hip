// ikpso_inst_contacts_serial_a.hip -- the contacts kernels (ikpso_solver_evaluate_contacts) of serial chains of 6, 7, 8 joints with a tip effector.
#define IKPSO_EVAL_KIND EvalContacts
#include "ikpso_evallist_serial_a.h"
