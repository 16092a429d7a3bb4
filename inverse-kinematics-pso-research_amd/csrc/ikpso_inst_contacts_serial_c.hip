// ikpso_inst_contacts_serial_c.hip -- the contacts kernels (ikpso_solver_evaluate_contacts) of serial chains of 12, 13, 14 joints with a tip effector.
#define IKPSO_EVAL_KIND EvalContacts
#include "ikpso_evallist_serial_c.h"
