// ikpso_inst_contacts_serial_b.hip -- the contacts kernels (ikpso_solver_evaluate_contacts) of serial chains of 9, 10, 11 joints with a tip effector.
#define IKPSO_EVAL_KIND EvalContacts
#include "ikpso_evallist_serial_b.h"
