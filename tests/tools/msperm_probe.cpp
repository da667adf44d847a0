// msperm_probe.cpp -- the host arithmetic of the permutation nulls (atlasqtl_amd/csrc/aq_msperm_plan.h) as a stand-alone host
// program, for what the C ABI reaches only with a handle or with the environment: the check of the permutation rows that
// aq_prep_marginal_perm runs before any device call, and the planner with forced tile edge, PB and batch.  One request per
// line of standard input, one answer per line:
//   rows n r0,r1,... [r0,r1,... ...]                        -> "<rc> <message or ->"   (every row must hold n entries)
//   plan n p1 q masked ncu n_perm tile pb batch             -> "<rc> tile pb batch launches lds_bytes | <message>"
//     g++ -std=c++17 -I atlasqtl_amd/csrc tests/tools/msperm_probe.cpp -o msperm_probe
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "aq_msperm_plan.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    std::string err;
    if (what == "rows") {
      int n = 0;
      in >> n;
      std::vector<int32_t> perm;
      std::string row;
      int n_perm = 0;
      while (in >> row) {
        std::istringstream rs(row);
        std::string v;
        size_t got = 0;
        while (std::getline(rs, v, ',')) {
          perm.push_back((int32_t)std::stol(v));
          got++;
        }
        if (got != (size_t)n) {
          std::printf("-1 row %d holds %zu entries\n", n_perm, got);
          return 2;
        }
        n_perm++;
      }
      const int rc = aq_msperm_check_rows(perm.data(), n_perm, n, "probe", &err);
      std::printf("%d %s\n", rc, rc == AQ_OK ? "-" : err.c_str());
    } else if (what == "plan") {
      int n, p1, q, masked, ncu, n_perm, tile, pb, batch;
      in >> n >> p1 >> q >> masked >> ncu >> n_perm >> tile >> pb >> batch;
      aq_msperm_plan pl{};
      const int rc = aq_msperm_make_plan(n, p1, q, masked, ncu, n_perm, tile, pb, batch, "probe", &pl, &err);
      if (rc == AQ_OK)
        std::printf("0 %d %d %d %d %d\n", pl.tile, pl.pb, pl.batch, pl.launches, pl.lds_bytes);
      else
        std::printf("%d | %s\n", rc, err.c_str());
    } else if (!what.empty()) {
      std::printf("-1 unknown request\n");
      return 2;
    }
  }
  return 0;
}
