// aq_launch_la2.hip -- instances of the look-ahead sweep kernel with 2 trait tile(s) per workgroup (see aq_launch_la.h): the
// recurrence wave owns aq_la_nt3's tiles, or nine (NT / NT / 9; none in the diagnostic build, AQ_LA_TT2_REC9).
#include "aq_launch_la_unit.h"

int aq_la_unit_tt2(const AqLaRequest &rq, const AqLaRun &run) { return aq_la_unit<2, false, false>(rq, run); }
