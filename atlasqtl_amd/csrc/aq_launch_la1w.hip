// aq_launch_la1w.hip -- instances of the look-ahead sweep kernel for the wide sample split (WIDE: 9 <= C <= AQ_LA_CMAX parts,
// complete Y, one trait tile per workgroup, NT2 == NT, unchained; see aq_launch_la.h).
#include "aq_launch_la_unit.h"

int aq_la_unit_wide(const AqLaRequest &rq, const AqLaRun &run) { return aq_la_unit<1, false, true>(rq, run); }
