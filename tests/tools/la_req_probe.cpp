// tests/tools/la_req_probe.cpp -- prints the request order the look-ahead kernel's deep operand prefetch is built with
// (atlasqtl_amd/csrc/aq_la_req.h), for tests/test_host_logic.py: one line "i D last stream k index" per request position and
// one line "n D last t issued" per step, for every depth, tile count, stream and tile.  Host compiler only.
#include <cstdio>
#include "aq_la_req.h"

int main() {
  for (int D = 2; D <= 4; D++)
    for (int last = 0; last <= 17; last++)
      for (int k = 0; k <= last; k++) {
        for (int stream = 0; stream < 2; stream++) std::printf("i %d %d %d %d %d\n", D, last, stream, k, aq_req_index(D, last, stream, k));
        std::printf("n %d %d %d %d\n", D, last, k, aq_req_issued(D, last, k));
      }
  return 0;
}
