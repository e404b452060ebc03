// ke_gang.h -- gang runs of a ke_schedule call (include/koord_eval.h, "gangs"), free of HIP and of the
// Context: the validation of ke_pod_gangs' runs, the per-pod gang word the replay reads, and the five rules of a run as
// a plain state machine.  ke_host.h and ke_kernels.hip include it; tests/gang/gang_check.cpp compiles it alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/koord_eval.h"

namespace ke {

// The gang word of a pod (one int32 a pod, the last section of the staging block): 0 = outside every run.
//   bit 0  member of a run          bit 1  the run's first member          bit 2  KE_GANG_STRICT
//   bits 8..23  need = max(min_member - assumed, 0), saturated (a run holds at most 64 members)
constexpr int32_t GW_MEMBER = 1, GW_FIRST = 2, GW_STRICT = 4;
constexpr int GW_NEED_SHIFT = 8;
constexpr int32_t GW_NEED_MAX = 0xFFFF;
inline int32_t gang_need(const ke_gang_run& r) {
  const int64_t need = (int64_t)r.min_member - (int64_t)r.assumed;
  return (int32_t)std::max<int64_t>(0, std::min<int64_t>(need, GW_NEED_MAX));
}
constexpr int32_t gw_need(int32_t w) { return (w >> GW_NEED_SHIFT) & GW_NEED_MAX; }
inline int32_t gang_word(const ke_gang_run& r, int32_t pos) {
  return GW_MEMBER | (pos == r.first ? GW_FIRST : 0) | (r.mode == KE_GANG_STRICT ? GW_STRICT : 0) |
         (gang_need(r) << GW_NEED_SHIFT);
}

// ke_pod_gangs' argument check: runs ascending and disjoint inside [0, n_pods), 1 <= count, min_member >= 1,
// assumed >= 0, a known mode, reserved == 0.  *why names the first violation.
inline int gang_validate(int32_t n_pods, int32_t n_runs, const ke_gang_run* runs, const char** why) {
  *why = "";
  if (n_pods < 0 || n_runs < 0 || (n_runs > 0 && !runs)) return *why = "ke_pod_gangs arguments", KE_ERR_INVALID;
  int64_t end = 0;
  for (int32_t i = 0; i < n_runs; i++) {
    const ke_gang_run& r = runs[i];
    if (r.count < 1) return *why = "ke_pod_gangs: a run of fewer than one pod", KE_ERR_INVALID;
    if (r.first < 0 || (int64_t)r.first + r.count > n_pods) return *why = "ke_pod_gangs: a run outside the call's pods", KE_ERR_INVALID;
    if (r.first < end) return *why = "ke_pod_gangs: runs overlap or are not ascending", KE_ERR_INVALID;
    if (r.min_member < 1) return *why = "ke_pod_gangs: min_member below 1", KE_ERR_INVALID;
    if (r.assumed < 0) return *why = "ke_pod_gangs: assumed below 0", KE_ERR_INVALID;
    if (r.mode != KE_GANG_STRICT && r.mode != KE_GANG_NON_STRICT) return *why = "ke_pod_gangs: mode", KE_ERR_INVALID;
    if (r.reserved != 0) return *why = "ke_pod_gangs: reserved must be 0", KE_ERR_INVALID;
    end = (int64_t)r.first + r.count;
  }
  return KE_OK;
}

// the words of a call's pods (validated runs)
inline std::vector<int32_t> gang_words(int32_t n_pods, int32_t n_runs, const ke_gang_run* runs) {
  std::vector<int32_t> w((size_t)n_pods, 0);
  for (int32_t i = 0; i < n_runs; i++)
    for (int32_t p = runs[i].first; p < runs[i].first + runs[i].count; p++) w[(size_t)p] = gang_word(runs[i], p);
  return w;
}
// members of the run that starts at p0 (words[p0] has GW_FIRST)
inline int32_t gang_run_len(const int32_t* words, int32_t n_pods, int32_t p0) {
  int32_t e = p0 + 1;
  while (e < n_pods && (words[e] & GW_MEMBER) && !(words[e] & GW_FIRST)) e++;
  return e - p0;
}

// The five rules (include/koord_eval.h) over a queue's gang words, one pod at a time in queue order.
//   place(p) -> node >= 0 or -1: schedules pod p on the current state (quota admission, Filter, Score, pick, Reserve)
//   undo(p, node): unreserves pod p from `node` (every plugin's Unreserve)
// Writes per pod the placement (-1: none), the status and the node a rolled-back member had (-1 otherwise).
struct GangCounts {
  int64_t runs = 0, rolled_back = 0, inverses = 0;
};
template <class Place, class Undo>
GangCounts gang_machine(int32_t n_pods, const int32_t* words, Place place, Undo undo, int32_t* chosen, int32_t* status,
                        int32_t* tried) {
  GangCounts cnt;
  int32_t first = 0, waiting = 0;
  bool failed = false, satisfied = false;
  for (int32_t p = 0; p < n_pods; p++) {
    const int32_t w = words ? words[p] : 0;
    tried[p] = -1;
    if (!(w & GW_MEMBER)) {
      chosen[p] = place(p);
      status[p] = KE_GANG_NONE;
      continue;
    }
    if (w & GW_FIRST) first = p, waiting = 0, failed = false, satisfied = gw_need(w) == 0, cnt.runs++;
    if (failed) {  // rule 1: PreFilter answers the context's failedMessage
      chosen[p] = -1, status[p] = KE_GANG_SKIPPED;
      continue;
    }
    chosen[p] = place(p);  // rule 2
    if (chosen[p] < 0) {   // rule 3: PostFilter
      status[p] = KE_GANG_FAILED;
      if (satisfied) continue;  // a satisfied run's later members are ordinary pods
      failed = true;
      if (!(w & GW_STRICT)) continue;
      cnt.rolled_back++;
      for (int32_t m = first; m < p; m++) {
        if (chosen[m] < 0) continue;
        undo(m, chosen[m]);
        tried[m] = chosen[m], chosen[m] = -1, status[m] = KE_GANG_ROLLED_BACK;
        cnt.inverses++;
      }
      continue;
    }
    waiting++;  // rule 4: Permit
    status[p] = satisfied ? KE_GANG_PLACED : KE_GANG_WAITING;  // rule 5 until the run is satisfied
    if (!satisfied && waiting >= gw_need(w)) {
      satisfied = true;
      for (int32_t m = first; m <= p; m++)
        if (status[m] == KE_GANG_WAITING) status[m] = KE_GANG_PLACED;
    }
  }
  return cnt;
}

}  // namespace ke
