// aq_launch_la1m.hip -- instances of the look-ahead sweep kernel for Y with missing values (MASK, one trait tile per workgroup;
// see aq_launch_la.h).  No residual tiles on the recurrence wave: aq_la_built (aq_plan_const.h) says why.
#include "aq_launch_la_unit.h"

int aq_la_unit_mask(const AqLaRequest &rq, const AqLaRun &run) { return aq_la_unit<1, true, false>(rq, run); }
