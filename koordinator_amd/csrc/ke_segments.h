// ke_segments.h — the level above one device call ("the segments of a ke_schedule call"): how ke_schedule
// cuts its queue into segments, one device_schedule each, and the one record their per-pod outputs are joined into.
// No HIP and no Context: tests/plan/segments_check.cpp compiles this header alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/koord_eval.h"

namespace ke {

// ---- the segment plan ------------------------------------------------------------------------------------------------
// What the cut needs of a pod.  PC_BARRIER: it Reserves into a limit_is_max quota with the runtime quota on (later pods
// see limits refreshed after it).  PC_ALONE: it has matched reservations (its rows carry its matched restore), or it
// ignores them and needs trials on the current state.  PC_IGNORED: KE_RSV_IGNORED (rows with every reservation's restore).
enum PodClass : uint8_t { PC_BARRIER = 1, PC_ALONE = 2, PC_IGNORED = 4 };

struct Segment {
  int32_t s0, s1;  // pods [s0, s1)
  bool ign;        // a run of KE_RSV_IGNORED pods
  bool alone;      // one PC_ALONE pod: a matched pod, or (ign) an ignored pod with its trials
  bool barrier;    // its last pod is a barrier
  bool matched() const { return alone && !ign; }
};

// A segment takes pods while they are no barrier, not alone and ignored as its first pod is.  The pod that stopped the
// walk joins an empty segment (an alone pod is a segment of one, also when it is a barrier), and a barrier that could
// have joined otherwise ends its segment inclusively.  An empty queue is one empty segment (the call still refreshes).
inline std::vector<Segment> plan_segments(int32_t n_pods, const uint8_t* cls) {
  std::vector<Segment> out;
  for (int32_t s0 = 0; s0 < n_pods || out.empty();) {
    const bool ign = s0 < n_pods && (cls[s0] & PC_IGNORED);
    auto joins = [&](int32_t p) { return !(cls[p] & PC_ALONE) && ((cls[p] & PC_IGNORED) != 0) == ign; };
    int32_t s1 = s0;
    while (s1 < n_pods && joins(s1) && !(cls[s1] & PC_BARRIER)) s1++;
    if (s1 < n_pods && (s1 == s0 || joins(s1))) s1++;
    out.push_back({s0, s1, ign, s1 - s0 == 1 && (cls[s0] & PC_ALONE), s1 > s0 && (cls[s1 - 1] & PC_BARRIER)});
    if (s1 == s0) break;
    s0 = s1;
  }
  return out;
}

// The static half of "fused" (DESIGN.md §4k): the pod after a plain segment may run last in the segment's call when it
// is a KE_RSV_MATCHED pod with matched reservations that neither binds CPUs nor requests devices (`next_plain`), on an
// unsharded context without a quota tree.  Whether it has views or decisions is known only on the segment's state.
inline bool may_fuse(const Segment& seg, bool next_matched, bool next_plain, bool quotas, bool sharded) {
  return !seg.ign && !seg.alone && seg.s1 > seg.s0 && next_matched && next_plain && !quotas && !sharded;
}

// ---- the record of a call's per-pod outputs -----------------------------------------------------------------------
// One device-made kind, W words a pod.  A kind none of a call's batches can make is not read back: the vector is empty
// and every pod reads as absent.
template <class T, size_t W>
struct PerPod {
  std::vector<T> v;
  const T* at(int64_t p) const { return p >= 0 && v.size() >= ((size_t)p + 1) * W ? v.data() + (size_t)p * W : nullptr; }
  void fill(const T* src, size_t n, bool has) { v.assign(src, src + (has ? n * W : 0)); }
  // a segment's first `len` pods behind this record's n: absent until a segment has the kind, then padded with `absent`
  void append(const PerPod& seg, size_t n, size_t len, T absent) {
    if (v.empty() && seg.v.empty()) return;
    v.resize(n * W, absent);
    v.insert(v.end(), seg.v.begin(), seg.v.begin() + (std::ptrdiff_t)std::min(seg.v.size(), len * W));
    v.resize((n + len) * W, absent);
  }
  void truncate(size_t len) { v.resize(std::min(v.size(), len * W)); }
  void flat(int64_t n_out, T* out) const {  // the ke_last_* view of the first n_out pods
    for (int64_t i = 0; i < n_out * (int64_t)W; i++) out[i] = i < (int64_t)v.size() ? v[(size_t)i] : 0;
  }
};

// The release records of one call (ke_last_allocations / ke_unreserve): per pod the chosen node (-1 once unreserved),
// the uid, whether its ElasticQuota Reserve ran, 1 + the reservation assumed (0 = none), the device-made allocations.
struct CallRecords {
  std::vector<int32_t> chosen, resv;
  std::vector<int64_t> uid;
  std::vector<uint8_t> quota;
  PerPod<uint64_t, 1> devs;                         // device minors (bit 16*type + minor)
  PerPod<uint64_t, 4> cpusets;                      // CPU-id bitset
  PerPod<int8_t, 2 * KE_MAX_MINORS> vfs;            // VF ranks [2][KE_MAX_MINORS], absent: -1
  PerPod<int64_t, KE_MAX_NUMA * KE_NRES> numas;     // NUMA amounts [2*id + r]
  PerPod<int32_t, 1> gang_status, gang_tried;       // KE_GANG_* and a rolled-back member's node (a call with gang runs)
  int64_t gang_counts[4] = {0, 0, 0, 0};            // ke_debug_gangs: runs, runs rolled back, inverse Reserves, cut batches
  // ke_debug_gang_devices: device inverses, cuts inside an open run, slots adopted, relaunches with a restored run state
  int64_t gang_dev_counts[4] = {0, 0, 0, 0};
  size_t n = 0;          // pods the device-made kinds cover
  int32_t resv_gen = 0;  // the reservation set `resv` indexes (ke_reservations_generation)
  // per pod: 0 / nullptr = absent
  uint64_t dev(int64_t p) const { return devs.at(p) ? *devs.at(p) : 0; }
  const uint64_t* cpuset(int64_t p) const { return cpusets.at(p); }
  const int8_t* vf(int64_t p) const { return vfs.at(p); }
  const int64_t* numa(int64_t p) const { return numas.at(p); }
  // a device call's completion: its np pods' read-back blocks, each kind present or not
  void fill_device(size_t np, const uint64_t* d, bool has_dev, const uint64_t* cs, bool has_cs, const int8_t* v, bool has_vf,
                   const int64_t* nu, bool has_numa) {
    devs.fill(d, np, has_dev), cpusets.fill(cs, np, has_cs), vfs.fill(v, np, has_vf), numas.fill(nu, np, has_numa);
    n = np;
  }
  void fill_gangs(size_t np, const int32_t* status, const int32_t* tried, bool has) {
    gang_status.fill(status, np, has), gang_tried.fill(tried, np, has);
    std::fill(gang_counts, gang_counts + 4, (int64_t)0);
    std::fill(gang_dev_counts, gang_dev_counts + 4, (int64_t)0);
  }
  void clear_device() {
    fill_device(0, nullptr, false, nullptr, false, nullptr, false, nullptr, false);
    fill_gangs(0, nullptr, nullptr, false);
  }
  void append(const CallRecords& seg, size_t len) {
    devs.append(seg.devs, n, len, 0), cpusets.append(seg.cpusets, n, len, 0);
    vfs.append(seg.vfs, n, len, -1), numas.append(seg.numas, n, len, 0);
    gang_status.append(seg.gang_status, n, len, 0), gang_tried.append(seg.gang_tried, n, len, -1);
    for (int i = 0; i < 4; i++) gang_counts[i] += seg.gang_counts[i], gang_dev_counts[i] += seg.gang_dev_counts[i];
    n += len;
  }
  // the call's pods: chosen node, uid, whether the ElasticQuota Reserve ran; `resv` keeps what the call assumed
  void set_pods(int32_t n_pods, const int32_t* ch, const ke_pod* pods, bool quota_tree, int32_t gen) {
    chosen.assign(ch, ch + n_pods), uid.resize((size_t)n_pods), quota.resize((size_t)n_pods), resv.resize((size_t)n_pods, 0);
    for (int32_t p = 0; p < n_pods; p++) uid[(size_t)p] = pods[p].uid, quota[(size_t)p] = quota_tree && ch[p] >= 0 && pods[p].quota > 0;
    resv_gen = gen;
  }
  void truncate(size_t len) {  // a gated fused pod: the segment's pods only
    devs.truncate(len), cpusets.truncate(len), vfs.truncate(len), numas.truncate(len);
    gang_status.truncate(len), gang_tried.truncate(len);
    n = std::min(n, len);
  }
  // ke_schedule_wait collects a call.  A reservation set loaded since names other reservations: `resv` drops them.
  void restore(CallRecords&& saved, int32_t gen_now) {
    *this = std::move(saved);
    if (resv_gen != gen_now) resv.assign(chosen.size(), 0), resv_gen = gen_now;
  }
  // ke_last_allocations' record of pod p; the reservation's uid and generation: of the loaded set
  ke_pod_allocation allocation(int64_t p, int32_t gen_now, const std::vector<ke_reservation>& set) const {
    ke_pod_allocation a{};
    std::fill(&a.vf_rank[0][0], &a.vf_rank[0][0] + 2 * KE_MAX_MINORS, (int8_t)-1);
    a.node = p < (int64_t)chosen.size() ? chosen[(size_t)p] : -1;
    if (a.node < 0) return a;
    a.reservation = p < (int64_t)resv.size() ? resv[(size_t)p] : 0;
    a.reservation_generation = gen_now;
    a.reservation_uid = a.reservation > 0 ? set[(size_t)a.reservation - 1].uid : 0;
    a.quota_assigned = quota[(size_t)p];
    if (const uint64_t* cs = cpuset(p)) std::copy(cs, cs + 4, a.cpuset);
    if (const int64_t* nu = numa(p)) std::copy(nu, nu + KE_MAX_NUMA * KE_NRES, a.numa);
    a.device_minors = dev(p);
    if (const int8_t* r = vf(p)) std::copy(r, r + 2 * KE_MAX_MINORS, &a.vf_rank[0][0]);
    return a;
  }
};

// The timing outputs of a call (ke_last_schedule_stats / ke_last_pod_latencies; call_stats writes a device call's into
// its context by name), joined over the segments.
struct CallTimes {
  double total_ms = 0;
  std::vector<double> batch_ms, pod_lat;
  void add(double ms, const std::vector<double>& batches, const std::vector<double>& lat) {
    total_ms += ms;
    batch_ms.insert(batch_ms.end(), batches.begin(), batches.end());
    pod_lat.insert(pod_lat.end(), lat.begin(), lat.end());
  }
};

}  // namespace ke
