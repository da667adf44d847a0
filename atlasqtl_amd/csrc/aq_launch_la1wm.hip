// aq_launch_la1wm.hip -- MASK instances (Y with missing values) of the wide sample split (see aq_launch_la1w.hip): no residual
// tiles on the recurrence wave, as in every MASK instance (aq_launch_la1m.hip).
#include "aq_launch_la_unit.h"

int aq_la_unit_wide_mask(const AqLaRequest &rq, const AqLaRun &run) { return aq_la_unit<1, true, true>(rq, run); }
