// ke_gang.h and plan_batches' gang rule alone (no HIP, no library): a line-driven driver for tests/test_gang_host.py,
// built with -fsanitize=address,undefined and run as a program.  One command a line on stdin, one answer line each;
// <runs> = N then N x (first count min_member assumed mode reserved):
//   validate P <runs>            gang_validate                                 -> rc
//   words P <runs>               gang_words                                    -> P words
//   plan P B <runs>              plan_batches over P plain pods with the words -> cuts n_batches then per batch "pods grouped"
//   same P B                     plan_batches without the argument, with nullptr and with all-zero words -> "1" when equal
//   machine P <runs> o[0..P)     gang_machine; o[p]: the node pod p gets when tried, -1 = placed nowhere
//                                -> P chosen, P status, P tried, runs rolled_back inverses, then the undo calls "p:node"
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
  const char* why = "";
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    int P = 0;
    in >> P;
    if (cmd == "validate") {
      const std::vector<ke_gang_run> runs = read_runs(in);
      std::printf("%d\n", gang_validate(P, (int32_t)runs.size(), runs.data(), &why));
    } else if (cmd == "words") {
      const std::vector<ke_gang_run> runs = read_runs(in);
      for (int32_t w : gang_words(P, (int32_t)runs.size(), runs.data())) std::printf("%d ", w);
      std::printf("\n");
    } else if (cmd == "plan") {
      int B = 0;
      in >> B;
      const std::vector<ke_gang_run> runs = read_runs(in);
      const std::vector<int32_t> w = gang_words(P, (int32_t)runs.size(), runs.data());
      const std::vector<DevPod> pods((size_t)P);
      int cuts = -1;
      const std::vector<Batch> b = plan_batches(pods.data(), P, B, true, false, nullptr, nullptr, nullptr, w.data(), &cuts);
      std::printf("%d %zu", cuts, b.size());
      for (const Batch& x : b) std::printf(" %d %d", x.pods, (int)x.grouped);
      std::printf("\n");
    } else if (cmd == "same") {
      int B = 0;
      in >> B;
      std::vector<DevPod> pods((size_t)P);
      for (int p = 0; p < P; p++) pods[(size_t)p].flags = p % 5 == 3 ? (uint32_t)PF_DS : 0u;  // (DeviceShare pods share batches)
      const std::vector<int32_t> zero((size_t)P, 0);
      int cuts = -1;
      const std::vector<Batch> a = plan_batches(pods.data(), P, B, true, false);
      const std::vector<Batch> b = plan_batches(pods.data(), P, B, true, false, nullptr, nullptr, nullptr, nullptr, &cuts);
      const std::vector<Batch> c = plan_batches(pods.data(), P, B, true, false, nullptr, nullptr, nullptr, zero.data(), &cuts);
      std::printf("%d\n", (int)(same_plan(a, b) && same_plan(a, c) && cuts == 0));
    } else if (cmd == "machine") {
      const std::vector<ke_gang_run> runs = read_runs(in);
      std::vector<int32_t> o((size_t)P), chosen((size_t)P), status((size_t)P), tried((size_t)P);
      for (int32_t& x : o) in >> x;
      const std::vector<int32_t> w = gang_words(P, (int32_t)runs.size(), runs.data());
      std::string undone;
      const GangCounts c = gang_machine(
          P, w.data(), [&](int32_t p) { return o[(size_t)p]; },
          [&](int32_t p, int32_t node) { undone += " " + std::to_string(p) + ":" + std::to_string(node); }, chosen.data(),
          status.data(), tried.data());
      for (int32_t x : chosen) std::printf("%d ", x);
      for (int32_t x : status) std::printf("%d ", x);
      for (int32_t x : tried) std::printf("%d ", x);
      std::printf("%lld %lld %lld%s\n", (long long)c.runs, (long long)c.rolled_back, (long long)c.inverses, undone.c_str());
    } else {
      std::printf("?\n");
    }
  }
  return 0;
}
