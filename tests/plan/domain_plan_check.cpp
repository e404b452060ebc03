// The spread domain part of the host plan (koordinator_amd/csrc/ke_plan.h) compiled alone for the host, for
// tests/test_spread_domains_plan.py.  Reads lines "B n  f_0 d_0 .. f_{n-1} d_{n-1}" (f as plan_check's segment mode:
// 1 PF_DS | 2 PF_CPUSET | 4 PF_DS_HINT; d the pod's spread domain group id) and prints, per line, two plans separated
// by '|' -- with the domain ids, then without them -- each as "pods ds cpu cut hint grouped" per batch, a '/', and
// run_end of (pipeline on, no NUMA, 100 nodes).
#include <cstdio>
#include <iostream>
#include <vector>

#include "../../koordinator_amd/csrc/ke_plan.h"

using namespace ke;

static int print_plan(const std::vector<DevPod>& pods, int B, const int32_t* dids) {
  const int n = (int)pods.size();
  const std::vector<Batch> bt =
      dids ? plan_batches(pods.data(), n, B, true, false, nullptr, dids) : plan_batches(pods.data(), n, B, true, false);
  const std::vector<int32_t> bases = plan_bases(bt);
  for (size_t b = 0; b < bt.size(); b++) {
    if (bases[b + 1] - bases[b] != bt[b].pods) return 1;
    std::printf("%d %d %d %d %d %d ", bt[b].pods, (int)bt[b].ds, (int)bt[b].cpu, (int)bt[b].cut, (int)bt[b].hint,
                (int)bt[b].grouped);
  }
  std::printf("/");
  for (int e : plan_runs(bt, true, 100, false, false)) std::printf(" %d", e);
  return 0;
}

int main() {
  int B, n;
  while (std::cin >> B >> n) {
    std::vector<DevPod> pods((size_t)n);  // (zeroed)
    std::vector<int32_t> dids((size_t)n);
    for (int p = 0; p < n; p++) {
      int f;
      std::cin >> f >> dids[(size_t)p];
      pods[(size_t)p].flags = (f & 1 ? PF_DS : 0u) | (f & 2 ? PF_CPUSET : 0u) | (f & 4 ? PF_DS_HINT : 0u);
    }
    if (print_plan(pods, B, dids.data())) return 1;
    std::printf(" | ");
    if (print_plan(pods, B, nullptr)) return 1;
    std::printf("\n");
  }
  return 0;
}
