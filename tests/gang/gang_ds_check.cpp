// plan_batches and plan_select with ke_set_gang_devices' switch, alone (no HIP, no library): a line-driven driver for
// tests/test_gang_devices_host.py, built with -fsanitize=address,undefined and run as a program.  One command a line on
// stdin, one answer line each; <runs> = N then N x (first count min_member assumed mode reserved); <ds> = P digits, 1 = a
// DeviceShare pod:
//   plan P B on <ds> <runs>   plan_batches with the words and the switch -> cuts n_batches then per batch
//                             "pods ds cut grouped"
//   off P B <ds> <runs>       the plan with the switch off, with the argument defaulted and with false -> "1" when equal
//   select N pods extra       plan_select of an exact-mode DeviceShare batch of `pods` pods -> L kext parts sorted
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../koordinator_amd/csrc/ke_plan.h"

using namespace ke;

static std::vector<ke_gang_run> read_runs(std::istream& in) {
  int n = 0;
  in >> n;
  std::vector<ke_gang_run> runs((size_t)(n > 0 ? n : 0));
  for (ke_gang_run& r : runs) in >> r.first >> r.count >> r.min_member >> r.assumed >> r.mode >> r.reserved;
  return runs;
}
static std::vector<DevPod> read_pods(std::istream& in, int P) {
  std::string ds;
  in >> ds;
  std::vector<DevPod> pods((size_t)P);
  for (int p = 0; p < P && p < (int)ds.size(); p++) pods[(size_t)p].flags = ds[(size_t)p] == '1' ? (uint32_t)PF_DS : 0u;
  return pods;
}
static bool same_plan(const std::vector<Batch>& a, const std::vector<Batch>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].pods != b[i].pods || a[i].ds != b[i].ds || a[i].cpu != b[i].cpu || a[i].cut != b[i].cut ||
        a[i].hint != b[i].hint || a[i].grouped != b[i].grouped)
      return false;
  return true;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "plan") {
      int P = 0, B = 0, on = 0;
      in >> P >> B >> on;
      const std::vector<DevPod> pods = read_pods(in, P);
      const std::vector<ke_gang_run> runs = read_runs(in);
      const std::vector<int32_t> w = gang_words(P, (int32_t)runs.size(), runs.data());
      int cuts = -1;
      const std::vector<Batch> b =
          plan_batches(pods.data(), P, B, true, false, nullptr, nullptr, nullptr, w.data(), &cuts, on != 0);
      std::printf("%d %zu", cuts, b.size());
      for (const Batch& x : b) std::printf(" %d %d %d %d", x.pods, (int)x.ds, (int)x.cut, (int)x.grouped);
      std::printf("\n");
    } else if (cmd == "off") {
      int P = 0, B = 0;
      in >> P >> B;
      const std::vector<DevPod> pods = read_pods(in, P);
      const std::vector<ke_gang_run> runs = read_runs(in);
      const std::vector<int32_t> w = gang_words(P, (int32_t)runs.size(), runs.data());
      int c0 = -1, c1 = -1;
      const std::vector<Batch> a = plan_batches(pods.data(), P, B, true, false, nullptr, nullptr, nullptr, w.data(), &c0);
      const std::vector<Batch> b = plan_batches(pods.data(), P, B, true, false, nullptr, nullptr, nullptr, w.data(), &c1, false);
      std::printf("%d\n", (int)(same_plan(a, b) && c0 == c1));
    } else if (cmd == "select") {
      int N = 0, pods = 0, extra = 0;
      in >> N >> pods >> extra;
      const Batch b{pods, true, false, pods > 1, false};
      const SelectPlan s = plan_select(N, b, SEL_EXACT, false, SelectKnob{}, extra);
      const SelectPlan z = plan_select(N, b, SEL_EXACT, false, SelectKnob{});
      std::printf("%d %d %d %d %d\n", s.L, s.kext, s.parts, (int)s.sorted, z.kext);
    } else {
      std::printf("?\n");
    }
  }
  return 0;
}
