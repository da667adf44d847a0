// aq_launch_la1.hip -- instances of the look-ahead sweep kernel with 1 trait tile(s) per workgroup (see aq_launch_la.h): the
// unsplit geometries with and without residual tiles on the recurrence wave, and the sample split's up to 18 tiles per wave.
#include "aq_launch_la_unit.h"

int aq_la_unit_tt1(const AqLaRequest &rq, const AqLaRun &run) { return aq_la_unit<1, false, false>(rq, run); }
