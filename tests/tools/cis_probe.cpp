// cis_probe.cpp -- the host arithmetic of the cis scan (atlasqtl_amd/csrc/aq_cis_plan.h) as a stand-alone host program, for
// what the C ABI does not hand out or reaches only with a handle or with the environment: the order of the traits and the
// list of work items, the check of the windows under an entry's name, and the planner with forced PB and batch.  One request
// per line of standard input, one answer per line:
//   plan n p1 q masked ncu n_perm pb batch lo0,lo1,... hi0,hi1,...
//     -> "0 | W trait_tiles q_active window_pairs staged_pairs lds perm_lds pb batch launches yp_bytes scratch_bytes | order |
//         tile_lo | tile_hi | first_item | item_tile | item_p0"   (lists comma-separated, "-" when empty)
//     -> "<rc> | <message>"
//     g++ -std=c++17 -I atlasqtl_amd/csrc tests/tools/cis_probe.cpp -o cis_probe
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "aq_cis_plan.h"

static std::vector<int32_t> parse_list(const std::string &s) {
  std::vector<int32_t> out;
  std::istringstream in(s);
  std::string v;
  while (std::getline(in, v, ',')) out.push_back((int32_t)std::stol(v));
  return out;
}

static void print_list(const std::vector<int32_t> &v) {
  std::printf(" | ");
  if (v.empty()) std::printf("-");
  for (size_t i = 0; i < v.size(); i++) std::printf(i ? ",%d" : "%d", v[i]);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "plan") {
      int n, p1, q, masked, ncu, n_perm, pb, batch;
      std::string slo, shi;
      in >> n >> p1 >> q >> masked >> ncu >> n_perm >> pb >> batch >> slo >> shi;
      const std::vector<int32_t> lo = parse_list(slo), hi = parse_list(shi);
      if (lo.size() != (size_t)q || hi.size() != (size_t)q) {
        std::printf("-1 | %zu and %zu bounds for %d traits\n", lo.size(), hi.size(), q);
        return 2;
      }
      aq_cis_plan pl{};
      aq_cis_work wk;
      std::string err;
      const int rc = aq_cis_make_plan(n, p1, q, masked, ncu, lo.data(), hi.data(), n_perm, pb, batch, "probe", &pl, &wk, &err);
      if (rc != AQ_OK) {
        std::printf("%d | %s\n", rc, err.c_str());
        continue;
      }
      std::printf("0 | %lld %d %d %lld %lld %d %d %d %d %d %lld %lld", (long long)pl.n_items, pl.trait_tiles, pl.q_active,
                  (long long)pl.window_pairs, (long long)pl.staged_pairs, pl.lds_bytes, pl.perm_lds_bytes, pl.pb, pl.batch, pl.launches,
                  (long long)pl.yp_bytes, (long long)pl.scratch_bytes);
      print_list(wk.order);
      print_list(wk.tile_lo);
      print_list(wk.tile_hi);
      print_list(wk.first_item);
      print_list(wk.item_tile);
      print_list(wk.item_p0);
      std::printf("\n");
    } else if (!what.empty()) {
      std::printf("-1 unknown request\n");
      return 2;
    }
  }
  return 0;
}
