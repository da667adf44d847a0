// plan_probe.cpp -- the launch planner (atlasqtl_amd/csrc/aq_plan.h) as a stand-alone host program, for the plan fields that
// aq_vb_status does not report: the generic kernel's (NE, WPT) and the SNP columns it stages at a time.
//   usage: plan_probe [ncu [total_bytes]] < rows
//   a row:  n p q max_missing max_short_list hooks      hooks: "-" or NAME=value,NAME=value
//   prints: use_tw NE WPT tw_ns n_pad                   or "error <code> <message>"
// Built by tests/test_fallback_coverage_host.py with the host compiler; no HIP, no device.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "aq_plan.h"

int main(int argc, char **argv) {
  const int ncu = argc > 1 ? atoi(argv[1]) : 256;
  const long long total = argc > 2 ? atoll(argv[2]) : 288LL * 1000 * 1000 * 1000;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream is(line);
    AqPlanInput in;
    std::string hooks;
    if (!(is >> in.n >> in.p >> in.q >> in.max_missing >> in.max_short_list >> hooks)) {
      std::printf("error -1 malformed row\n");
      return 2;
    }
    in.has_missing = in.max_missing > 0;
    in.ncu = ncu;
    in.total_bytes = total;
    std::vector<std::pair<std::string, std::string>> hk;
    if (hooks != "-") {
      std::istringstream hs(hooks);
      std::string item;
      while (std::getline(hs, item, ',')) {
        const size_t eq = item.find('=');
        if (eq == std::string::npos || eq == 0) {
          std::printf("error -1 malformed hook\n");
          return 2;
        }
        hk.push_back({item.substr(0, eq), item.substr(eq + 1)});
      }
    }
    const AqEnv env = [&hk](const char *name) -> const char * {
      for (auto &h : hk)
        if (h.first == name) return h.second.c_str();
      return nullptr;
    };
    AqPlan pl;
    std::string err;
    const int rc = aq_make_plan(in, env, &pl, &err);
    if (rc != AQ_OK) std::printf("error %d %s\n", rc, err.c_str());
    else std::printf("%d %d %d %d %d\n", pl.use_tw ? 1 : 0, pl.NE, pl.WPT, pl.tw_ns, pl.n_pad);
  }
  return 0;
}
