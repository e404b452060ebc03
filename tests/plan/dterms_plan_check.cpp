// plan_batches' cut rule for spread domain term lists (koordinator_amd/csrc/ke_plan.h) compiled alone
// for the host, for tests/test_spread_domain_terms_plan.py.  Reads lines
//   B n  then per pod:  nt g_1 .. g_nt  nm m_1 .. m_nm      (the groups of the pod's terms, its member groups)
// and prints per line three plans, each behind a '|': with the lists (marks: the pods with a non-empty list), without
// any attachment, and with §4s ids (a pod whose lists are exactly one term on g and the member g has id g, else 0) --
// each plan as "pods grouped" pairs, then "/" and plan_runs' run_end for a pipelined context of 100 nodes.
#include <cstdio>
#include <iostream>
#include <vector>

#include "../../koordinator_amd/csrc/ke_plan.h"

using namespace ke;

static void print_plan(const std::vector<Batch>& bt) {
  std::printf("|");
  for (const Batch& b : bt) std::printf(" %d %d", b.pods, (int)b.grouped);
  std::printf(" /");
  for (int e : plan_runs(bt, true, 100, false, false)) std::printf(" %d", e);
  std::printf(" ");
}

int main() {
  int B, n;
  while (std::cin >> B >> n) {
    std::vector<DevPod> pods((size_t)n);  // (zeroed: plain pods)
    std::vector<PodTerms> recs((size_t)n, PodTerms{});
    std::vector<int32_t> listed((size_t)n, 0), ids((size_t)n, 0);
    for (int p = 0; p < n; p++) {
      int nt, nm, g;
      std::cin >> nt;
      if (nt > POD_TERMS) return 1;
      for (int t = 0; t < nt; t++) {
        std::cin >> g;
        recs[(size_t)p].tw[t] = (uint32_t)g | (uint32_t)ST_SKEW << 16;
      }
      std::cin >> nm;
      if (nm > POD_MEMBERS) return 1;
      for (int m = 0; m < nm; m++) {
        std::cin >> g;
        recs[(size_t)p].mem[m >> 1] |= (uint32_t)g << ((m & 1) * 16);
      }
      listed[(size_t)p] = st_empty(recs[(size_t)p]) ? 0 : 1;
      if (nt == 1 && nm == 1 && st_group(recs[(size_t)p], 0) == st_member(recs[(size_t)p], 0)) ids[(size_t)p] = g;
    }
    print_plan(plan_batches(pods.data(), n, B, true, false, listed.data(), nullptr, recs.data()));
    print_plan(plan_batches(pods.data(), n, B, true, false));
    print_plan(plan_batches(pods.data(), n, B, true, false, nullptr, ids.data()));
    std::printf("\n");
  }
  return 0;
}
