// The host half of ke_preempt, free of HIP: the resident-pod table (a statement by the caller: per
// node its pods in util.MoreImportantPod order, with the checks and caps of every entry point), its packing into the
// device copy (a CSR of 32-byte records in list order), the per-preemptor uniforms the host computes, the raw class
// tallies and the lexicographic key of the pick.  ke_kernels.hip and ke_capi.cpp include it;
// tests/preempt/preempt_check.cpp compiles it alone with g++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/koord_eval.h"

#ifndef KE_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define KE_HD __host__ __device__
#else
#define KE_HD
#endif
#endif

namespace ke {

// ---- the order ---------------------------------------------------------------------------------------------------------
// util.MoreImportantPod (upstream k8s, outside the reference tree: restated, parity-unpinned): the higher priority
// first, then the earlier start time; what sort.Slice would leave unordered goes by uid ascending (a convention).
inline bool resident_before(const ke_resident_pod& a, const ke_resident_pod& b) {
  if (a.priority != b.priority) return a.priority > b.priority;
  if (a.start_ns != b.start_ns) return a.start_ns < b.start_ns;
  return a.uid < b.uid;
}

constexpr int64_t RESIDENT_CPU_LIMIT = 1LL << 47;  // the device record keeps cpu (milli) in 48 bits

// One record's own fields (KE_OK, or KE_ERR_INVALID with *why).
inline int resident_check(const ke_resident_pod& r, const char** why) {
  for (int q = 0; q < KE_NRES; q++)
    if (r.requests[q] < 0) return *why = "ke_resident_pod.requests must be >= 0", KE_ERR_INVALID;
  if (r.requests[KE_RES_CPU] >= RESIDENT_CPU_LIMIT) return *why = "ke_resident_pod cpu request at or above 2^47", KE_ERR_INVALID;
  if (r.quota < 0 || r.quota > KE_MAX_QUOTAS) return *why = "ke_resident_pod.quota outside 0..KE_MAX_QUOTAS", KE_ERR_INVALID;
  if (r.non_preemptible > 1) return *why = "ke_resident_pod.non_preemptible must be 0 or 1", KE_ERR_INVALID;
  if (r.n_pdb > 2) return *why = "ke_resident_pod.n_pdb above 2", KE_ERR_INVALID;
  for (int j = 0; j < r.n_pdb; j++)
    if (r.pdb[j] == 0) return *why = "ke_resident_pod.pdb id 0 within n_pdb", KE_ERR_INVALID;
  if (r.n_pdb == 2 && r.pdb[0] == r.pdb[1]) return *why = "ke_resident_pod names one pdb twice", KE_ERR_INVALID;
  return KE_OK;
}

// ---- the table ---------------------------------------------------------------------------------------------------------
struct ResidentTable {
  std::vector<std::vector<ke_resident_pod>> nodes;  // [node capacity], each list sorted by resident_before
  int64_t total = 0;
  bool dirty = true;  // the device copy is older than this table
};

inline int32_t resident_capacity(const ResidentTable& t) { return (int32_t)t.nodes.size(); }

// ke_resident_pods_load: the whole table replaced (nothing changes on a refusal).
inline int resident_load(ResidentTable& t, int32_t n_nodes, const int32_t* off, const ke_resident_pod* pods, const char** why) {
  if (n_nodes < 0 || n_nodes > resident_capacity(t)) return *why = "ke_resident_pods_load: n_nodes outside 0..node_capacity", KE_ERR_INVALID;
  if (n_nodes > 0 && !off) return *why = "ke_resident_pods_load: null offsets", KE_ERR_INVALID;
  if (n_nodes > 0 && off[0] != 0) return *why = "ke_resident_pods_load: offsets[0] must be 0", KE_ERR_INVALID;
  for (int32_t i = 0; i < n_nodes; i++) {
    if (off[i + 1] < off[i]) return *why = "ke_resident_pods_load: offsets must not decrease", KE_ERR_INVALID;
    if (off[i + 1] - off[i] > KE_MAX_RESIDENT_PODS) return *why = "more than KE_MAX_RESIDENT_PODS resident pods on a node", KE_ERR_UNSUPPORTED;
  }
  const int64_t n = n_nodes > 0 ? off[n_nodes] : 0;
  if (n > 0 && !pods) return *why = "ke_resident_pods_load: null pods", KE_ERR_INVALID;
  for (int64_t j = 0; j < n; j++) {
    const int rc = resident_check(pods[j], why);
    if (rc) return rc;
  }
  std::vector<std::vector<ke_resident_pod>> next(t.nodes.size());
  for (int32_t i = 0; i < n_nodes; i++) {
    std::vector<ke_resident_pod>& l = next[(size_t)i];
    l.assign(pods + off[i], pods + off[i + 1]);
    std::sort(l.begin(), l.end(), resident_before);
    // (equal uids are neighbours only when priority and start agree too: look for them by uid)
    std::vector<int64_t> u(l.size());
    for (size_t j = 0; j < l.size(); j++) u[j] = l[j].uid;
    std::sort(u.begin(), u.end());
    if (std::adjacent_find(u.begin(), u.end()) != u.end()) return *why = "a uid listed twice on a node", KE_ERR_INVALID;
  }
  t.nodes.swap(next);
  t.total = n;
  t.dirty = true;
  return KE_OK;
}

inline int resident_add(ResidentTable& t, int32_t node, const ke_resident_pod* pod, const char** why) {
  if (node < 0 || node >= resident_capacity(t)) return *why = "node index out of range", KE_ERR_NOT_FOUND;
  if (!pod) return *why = "ke_resident_pod_add: null pod", KE_ERR_INVALID;
  const int rc = resident_check(*pod, why);
  if (rc) return rc;
  std::vector<ke_resident_pod>& l = t.nodes[(size_t)node];
  for (const ke_resident_pod& r : l)
    if (r.uid == pod->uid) return *why = "ke_resident_pod_add: the uid is already listed on the node", KE_ERR_INVALID;
  if ((int)l.size() >= KE_MAX_RESIDENT_PODS) return *why = "more than KE_MAX_RESIDENT_PODS resident pods on a node", KE_ERR_UNSUPPORTED;
  l.insert(std::upper_bound(l.begin(), l.end(), *pod, resident_before), *pod);
  t.total++;
  t.dirty = true;
  return KE_OK;
}

inline int resident_remove(ResidentTable& t, int32_t node, int64_t uid, const char** why) {
  if (node < 0 || node >= resident_capacity(t)) return *why = "node index out of range", KE_ERR_NOT_FOUND;
  std::vector<ke_resident_pod>& l = t.nodes[(size_t)node];
  for (size_t j = 0; j < l.size(); j++)
    if (l[j].uid == uid) {
      l.erase(l.begin() + (long)j);
      t.total--;
      t.dirty = true;
      return KE_OK;
    }
  return *why = "ke_resident_pod_remove: no such uid on the node", KE_ERR_NOT_FOUND;
}

// ke_node_delete: the node's list goes with it
inline void resident_drop(ResidentTable& t, int32_t node) {
  if (node < 0 || node >= resident_capacity(t) || t.nodes[(size_t)node].empty()) return;
  t.total -= (int64_t)t.nodes[(size_t)node].size();
  t.nodes[(size_t)node].clear();
  t.dirty = true;
}

inline int resident_get(const ResidentTable& t, int32_t node, int32_t cap, ke_resident_pod* out, int32_t* n, const char** why) {
  if (node < 0 || node >= resident_capacity(t)) return *why = "node index out of range", KE_ERR_NOT_FOUND;
  if (!n || cap < 0 || (cap > 0 && !out)) return *why = "ke_resident_pods_get arguments", KE_ERR_INVALID;
  const std::vector<ke_resident_pod>& l = t.nodes[(size_t)node];
  *n = (int32_t)l.size();
  for (int32_t j = 0; j < cap && j < *n; j++) out[j] = l[(size_t)j];
  return KE_OK;
}

// ---- the device copy ---------------------------------------------------------------------------------------------------
// One resident pod as the kernels read it: 32 bytes, two 16-byte loads a lane.  The uid is not part of it (only the
// victim list names pods): it lies in a parallel array.
struct DevResident {
  int64_t start_ns;
  int64_t mem;
  uint64_t cpu_pdb0;  // cpu (milli) in bits 0..47, pdb[0] (0 = none) in bits 48..63
  int32_t priority;
  uint16_t pdb1;      // pdb[1], 0 = none
  uint8_t quota;
  uint8_t flags;      // RF_*
};
static_assert(sizeof(DevResident) == 32, "a resident record is 32 bytes");
constexpr uint8_t RF_NON_PREEMPTIBLE = 1;
KE_HD inline int64_t dr_cpu(const DevResident& r) { return (int64_t)(r.cpu_pdb0 & ((1ull << 48) - 1)); }
KE_HD inline uint32_t dr_pdb0(const DevResident& r) { return (uint32_t)(r.cpu_pdb0 >> 48); }

// The CSR of the first n_nodes lists (offsets n_nodes + 1, records and uids in list order).  A pdb id beyond the
// loaded PDBs is refused here, at the call that would read it.
inline int resident_pack(const ResidentTable& t, int32_t n_nodes, int32_t n_pdbs, std::vector<int32_t>& off,
                         std::vector<DevResident>& rec, std::vector<int64_t>& uid, const char** why) {
  n_nodes = std::min(n_nodes, resident_capacity(t));
  off.assign((size_t)n_nodes + 1, 0);
  rec.clear();
  uid.clear();
  rec.reserve((size_t)t.total);
  uid.reserve((size_t)t.total);
  for (int32_t i = 0; i < n_nodes; i++) {
    for (const ke_resident_pod& r : t.nodes[(size_t)i]) {
      DevResident d{};
      d.start_ns = r.start_ns;
      d.mem = r.requests[KE_RES_MEMORY];
      const uint32_t p0 = r.n_pdb > 0 ? r.pdb[0] : 0u, p1 = r.n_pdb > 1 ? r.pdb[1] : 0u;
      if ((int64_t)p0 > n_pdbs || (int64_t)p1 > n_pdbs) return *why = "a resident pod names a pdb beyond ke_pdbs_load's array", KE_ERR_INVALID;
      d.cpu_pdb0 = (uint64_t)r.requests[KE_RES_CPU] | ((uint64_t)p0 << 48);
      d.priority = r.priority;
      d.pdb1 = (uint16_t)p1;
      d.quota = (uint8_t)r.quota;
      d.flags = r.non_preemptible ? RF_NON_PREEMPTIBLE : 0;
      rec.push_back(d);
      uid.push_back(r.uid);
    }
    off[(size_t)i + 1] = (int32_t)rec.size();
  }
  return KE_OK;
}

// ---- what the host computes per preemptor -------------------------------------------------------------------------------
// The priority, and the ElasticQuota figures of the reprieve's quota check (plugin.go:57-73's PostFilterState of the
// pod's quota at the call): used, the used limit on the keys it has, and the pod's own request masked by the quota's
// Max names as ke_schedule's admission masks it.  quota 0 is the skip state.
struct PreemptPod {
  int64_t used[KE_NRES], lim[KE_NRES], req[KE_NRES];
  int32_t priority;
  int16_t quota;         // as ke_pod.quota
  uint8_t lim_has;       // bit r: the used limit has resource r
  uint8_t max_has;       // bit r: the quota's Max names resource r (the mask of a victim's request)
  int16_t blocked_quota; // a victim of this quota (1 + index) is never preempted (DisableDefaultQuotaPreemption); 0 = none
  int16_t pad[3];
};
static_assert(sizeof(PreemptPod) == 64, "a preemptor's uniforms are 64 bytes");

// ---- the raw tallies: PRE_WORDS uint32 per pod, zeroed by the host before the launch ------------------------------------
constexpr int PRE_CANDIDATE = 0, PRE_SKIPPED = 1, PRE_NO_VICTIMS = 2, PRE_UNFIT = 3, PRE_ERROR = 4, PRE_ABSENT = 5, PRE_WORDS = 8;

// ---- the pick ----------------------------------------------------------------------------------------------------------
// A candidate's six criteria as one key, the smaller the better, compared word by word (pickOneNodeForPreemption,
// upstream k8s, outside the reference tree: restated, parity-unpinned):
//   w[0] = PDB violations << 32 | the highest victim priority (biased to unsigned)
//   w[1] = the sum of (priority + 2^31 + 1) over the victims (< 2^40 for 128 victims) << 8 | the victim count
//   w[2] = the complement of the earliest start among the highest-priority victims (biased): the latest start first
//   w[3] = the node index
// A candidate without victims has priority INT32_MIN and start INT64_MAX.  All ones in every word: no candidate.
struct PreemptKey {
  uint64_t w[4];
};
KE_HD inline PreemptKey preempt_key_none() { return PreemptKey{{~0ull, ~0ull, ~0ull, ~0ull}}; }
KE_HD inline bool preempt_key_is_none(const PreemptKey& k) { return k.w[3] == ~0ull; }
KE_HD inline PreemptKey preempt_key(int32_t violations, int32_t hi_prio, uint64_t prio_sum, int32_t n_victims,
                                    int64_t hi_start, int32_t node) {
  PreemptKey k;
  k.w[0] = ((uint64_t)(uint32_t)violations << 32) | (uint32_t)((uint32_t)hi_prio ^ 0x80000000u);
  k.w[1] = (prio_sum << 8) | (uint64_t)(uint32_t)n_victims;
  k.w[2] = ~((uint64_t)hi_start ^ (1ull << 63));
  k.w[3] = (uint64_t)(uint32_t)node;
  return k;
}
KE_HD inline bool preempt_key_less(const PreemptKey& a, const PreemptKey& b) {
  if (a.w[0] != b.w[0]) return a.w[0] < b.w[0];
  if (a.w[1] != b.w[1]) return a.w[1] < b.w[1];
  if (a.w[2] != b.w[2]) return a.w[2] < b.w[2];
  return a.w[3] < b.w[3];
}
KE_HD inline int32_t preempt_key_node(const PreemptKey& k) { return (int32_t)(uint32_t)k.w[3]; }
KE_HD inline int32_t preempt_key_victims(const PreemptKey& k) { return (int32_t)(k.w[1] & 0xFF); }
KE_HD inline int32_t preempt_key_violations(const PreemptKey& k) { return (int32_t)(k.w[0] >> 32); }

}  // namespace ke
