// ke_diagnose's host half (koordinator_amd/csrc/ke_diag.h) compiled alone for the host: folds hand-made raw tallies
// read from stdin and prints the ke_pod_diagnosis, for tests/test_diagnose_host.py to compare.  Modes:
//   fold  < lines   "n_slots absent feasible unschedulable unresolvable error  reason:count ..." per line ->
//                   "ok n_nodes n_absent n_feasible n_unschedulable n_unresolvable n_error plugins reason0 sum_rest"
//   tables          "reason plugin message" for every reason 0 .. KE_DIAG_REASONS - 1
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../koordinator_amd/csrc/ke_diag.h"

using namespace ke;

static int fold() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    uint32_t raw[DIAG_WORDS];
    std::memset(raw, 0, sizeof(raw));
    int n_slots = 0;
    in >> n_slots >> raw[DIAG_ABSENT] >> raw[DIAG_FEASIBLE] >> raw[DIAG_UNSCHEDULABLE] >> raw[DIAG_UNRESOLVABLE] >>
        raw[DIAG_ERROR];
    std::string tok;
    while (in >> tok) {
      int r = 0;
      unsigned c = 0;
      if (std::sscanf(tok.c_str(), "%d:%u", &r, &c) != 2 || r < 0 || r >= KE_DIAG_REASONS) return 2;
      raw[r] += c;
    }
    ke_pod_diagnosis d;
    const bool ok = diag_fold(raw, n_slots, &d);
    long rest = 0;
    for (int r = 1; r < KE_DIAG_REASONS; r++) rest += d.reason_nodes[r];
    std::printf("%d %d %d %d %d %d %d %u %d %ld\n", (int)ok, d.n_nodes, d.n_absent, d.n_feasible, d.n_unschedulable,
                d.n_unresolvable, d.n_error, d.plugins, d.reason_nodes[0], rest);
  }
  return 0;
}

static int tables() {
  for (int r = 0; r < KE_DIAG_REASONS; r++) std::printf("%d %u %s\n", r, diag_reason_plugin(r), diag_reason_message(r));
  return 0;
}

int main(int argc, char** argv) {
  static_assert(sizeof(ke_pod_diagnosis) == 32 + 4 * KE_DIAG_REASONS, "ke_pod_diagnosis layout");
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "fold") return fold();
  if (mode == "tables") return tables();
  return 64;
}
