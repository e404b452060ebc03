// A call's per-pod attachments ("the staging block"), free of HIP: the kinds a call can carry --
// node set ids (§4o), score table ids (§4p), spread group ids (§4r), spread domain group ids (§4s), spread term
// records (§4t), spread domain term records (§4u) and gang words (§4w) -- from their staging to the kernel mode, the
// upload layout and the host's share of the Reserves.
// ke_host.h and ke_kernels.hip include it; tests/plan/attach_check.cpp compiles it alone with g++.
#pragma once
#include <stdint.h>

#include <cstddef>
#include <vector>

#include "../../include/koord_eval.h"
#include "ke_types.h"

namespace ke {

// NS, the template mode of every kernel that makes a score or key: 0 = the call has no per-pod ids, NS_SETS = its
// ns_ids words are node set ids, NS_SCORES = they are (score table id << 16) | node set id, NS_GROUPS = NS_SCORES and
// the pods' spread groups (sg_ids) besides, NS_DOMAINS = NS_GROUPS and the pods' spread domain groups (sd_ids),
// NS_TERMS = NS_DOMAINS and the pods' spread term records (st_rec), NS_DTERMS = NS_TERMS and the pods' spread domain
// term records (dt_rec) with their per-domain tables (dt_tbl)
constexpr int NS_SETS = 1, NS_SCORES = 2, NS_GROUPS = 3, NS_DOMAINS = 4, NS_TERMS = 5, NS_DTERMS = 6;
// the modes whose kernels read the pods' spread domain ids and masks: a call with domain term lists carries no such id,
// so NS_DTERMS -- a superset of NS_TERMS otherwise -- leaves the §4s sites out
constexpr bool ns_sd(int ns) { return ns == NS_DOMAINS || ns == NS_TERMS; }

// One kind's staging slot: what its ke_pod_* entry point staged for the next call (`on`: staged, also when every id is
// 0 or every list empty) and what the call in progress took.
template <class T>
struct AttachSlot {
  std::vector<T> staged, call;
  bool on = false;
  void stage(const T* v, int32_t n) {
    staged.assign(v, v + n);
    on = true;
  }
  void stage(std::vector<T>& v) {
    staged.swap(v);
    on = true;
  }
  // the staging becomes the call's, consumed whether the call goes on or not; returns whether anything was staged
  bool take() {
    const bool was = on;
    call.clear();
    if (was) call.swap(staged);
    staged.clear();
    on = false;
    return was;
  }
};

// What the call in progress carries: per kind its per-pod array, nullptr where the call has no non-zero id / no
// non-empty list of that kind (it then runs the kernels it ran without the kind).  A call with term lists carries no
// spread group ids, a call with domain term lists neither those nor spread domain ids; listed[p] != 0 where pod p's
// term record or domain term record is not empty.
struct CallAttach {
  const int32_t* sets = nullptr;
  const int32_t* scores = nullptr;
  const int32_t* groups = nullptr;
  const int32_t* domains = nullptr;
  const PodTerms* terms = nullptr;
  const PodTerms* dterms = nullptr;
  // the gang words of the call's pods (ke_gang.h; nullptr: no run).  Not a kernel mode: the words stay
  // outside the ns() chain, and only the gang batches' Reserve kernel reads them.
  const int32_t* gangs = nullptr;
  std::vector<int32_t> listed;
  int32_t n_pods = 0;  // the pod count every array present was checked against

  void reset() {
    sets = scores = groups = domains = gangs = nullptr;
    terms = dterms = nullptr;
    listed.clear();
    n_pods = 0;
  }
  // the mode of the call's kernels: a later kind's kernels read the earlier kinds' tables too (row 0 at least)
  int ns() const { return dterms ? NS_DTERMS : terms ? NS_TERMS : domains ? NS_DOMAINS : groups ? NS_GROUPS : scores ? NS_SCORES : sets ? NS_SETS : 0; }
  // ... without the score tables, which do not filter (ke_diagnose)
  int ns_filter() const { return dterms ? NS_DTERMS : terms ? NS_TERMS : domains ? NS_DOMAINS : groups ? NS_GROUPS : sets ? NS_SETS : 0; }
  // ... of one batch of a ke_schedule call: a batch without a grouped pod keeps the set / score mode
  int batch_ns(bool grouped) const {
    return !grouped ? (scores ? NS_SCORES : sets ? NS_SETS : 0)
           : dterms ? NS_DTERMS : terms ? NS_TERMS : domains ? NS_DOMAINS : NS_GROUPS;
  }
  // plan_batches' marks: term lists and domain term lists mark a batch as group ids do
  const int32_t* plan_groups() const { return terms || dterms ? listed.data() : groups; }
  const int32_t* plan_domains() const { return domains; }
  // ... and its cut rule for domain term lists
  const PodTerms* plan_dterms() const { return dterms; }
};

// The staging block behind a call's DevPod records, in int32 words: the offset of each section the
// call has (-1: none) and their total.
struct AttachLayout {
  static constexpr int TERM_WORDS = sizeof(PodTerms) / sizeof(int32_t);
  static_assert(TERM_WORDS == 8 && sizeof(PodTerms) % sizeof(int32_t) == 0, "a term record is 8 words");
  int64_t ids = -1;      // the packed word: node set id | score table id << 16
  int64_t groups = -1;   // spread group ids
  int64_t domains = -1;  // spread domain group ids
  int64_t terms = -1;    // spread term records
  int64_t dterms = -1;   // spread domain term records
  int64_t gangs = -1;    // gang words (behind every other section: their offsets are those of a call without runs)
  int64_t total = 0;
  AttachLayout(const CallAttach& a, int64_t n_pods) {
    const bool dt = a.dterms, st = dt || a.terms, sd = st || a.domains, sg = sd || a.groups, id = sg || a.sets || a.scores;
    if (id) ids = total, total += n_pods;
    if (sg) groups = total, total += n_pods;
    if (sd) domains = total, total += n_pods;
    if (st) terms = total, total += TERM_WORDS * n_pods;
    if (dt) dterms = total, total += TERM_WORDS * n_pods;
    if (a.gangs) gangs = total, total += n_pods;
  }
};

// What a call's completion keeps of its attachments once the context has gone on to the next call: the kinds whose
// Reserves change the host tables.
struct PlacedAttach {
  std::vector<int32_t> groups, domains;
  std::vector<PodTerms> terms, dterms;
  PlacedAttach() = default;
  PlacedAttach(const CallAttach& a, int32_t n_pods) {
    if (a.groups) groups.assign(a.groups, a.groups + n_pods);
    if (a.domains) domains.assign(a.domains, a.domains + n_pods);
    if (a.terms) terms.assign(a.terms, a.terms + n_pods);
    if (a.dterms) dterms.assign(a.dterms, a.dterms + n_pods);
  }
};

// The increments the device's Reserves made, on the host copies of the tables (placements of an unsharded context:
// chosen[p] is the node index, -1 = not placed).  Writes ctx's sg_cnt / sd_cnt (Context, or a test's stand-in).
template <class Ctx>
void apply_placements(Ctx& ctx, const PlacedAttach& a, const int32_t* chosen) {
  for (size_t p = 0; p < a.groups.size(); p++) {
    const int32_t g = a.groups[p], node = chosen[p];
    if (g > 0 && g <= ctx.sg_n && node >= 0 && (int64_t)node < ctx.sg_stride)
      ctx.sg_cnt[(size_t)((int64_t)(g - 1) * ctx.sg_stride + node)]++;
  }
  // spread terms: every member of a placement, saturating as the device's Reserve does
  for (size_t p = 0; p < a.terms.size(); p++) {
    const int32_t node = chosen[p];
    if (node < 0 || (int64_t)node >= ctx.sg_stride) continue;
    for (int m = 0; m < POD_MEMBERS; m++) {
      const int g = st_member(a.terms[p], m);
      if (g < 1 || g > ctx.sg_n) continue;
      uint16_t& v = ctx.sg_cnt[(size_t)((int64_t)(g - 1) * ctx.sg_stride + node)];
      if (v < 65535) v++;
    }
  }
  // spread domains: the count of the placement's domain in the group's map
  for (size_t p = 0; p < a.domains.size(); p++) {
    const int32_t g = a.domains[p], node = chosen[p];
    if (g < 1 || g > ctx.sd_n || node < 0 || (int64_t)node >= ctx.sd_stride) continue;
    const uint16_t dom = ctx.sd_map[(size_t)((int64_t)(ctx.sd_gmap[(size_t)g - 1] - 1) * ctx.sd_stride + node)];
    if (dom < KE_MAX_SPREAD_DOMAINS) ctx.sd_cnt[(size_t)(g - 1) * KE_MAX_SPREAD_DOMAINS + dom]++;
  }
  // spread domain terms: for every member of a placement the count of the placement's domain in the member's map
  for (size_t p = 0; p < a.dterms.size(); p++) {
    const int32_t node = chosen[p];
    if (node < 0 || (int64_t)node >= ctx.sd_stride) continue;
    for (int m = 0; m < POD_MEMBERS; m++) {
      const int g = st_member(a.dterms[p], m);
      if (g < 1 || g > ctx.sd_n) continue;
      const uint16_t dom = ctx.sd_map[(size_t)((int64_t)(ctx.sd_gmap[(size_t)g - 1] - 1) * ctx.sd_stride + node)];
      if (dom < KE_MAX_SPREAD_DOMAINS) ctx.sd_cnt[(size_t)(g - 1) * KE_MAX_SPREAD_DOMAINS + dom]++;
    }
  }
}

}  // namespace ke
