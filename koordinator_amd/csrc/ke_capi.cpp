// ke_capi.cpp — the extern "C" boundary (include/koord_eval.h) over the host state (ke_host.cpp)
// and the device evaluator (ke_kernels.hip).
#include <algorithm>
#include <chrono>
#include <cstring>
#include <deque>
#include <new>

#include "ke_diag.h"
#include "ke_host.h"

namespace ke {
const char* last_error_cstr();
int device_available();
int device_create(Context* ctx);
void device_destroy(Context* ctx);
int device_eval(Context* ctx, int32_t n_pods, const ke_pod* pods, int64_t now, uint8_t* status, uint8_t* reason,
                int16_t* la, int16_t* numa, int16_t* ds, int16_t* total, int32_t* best);
int device_diagnose(Context* ctx, int32_t n_pods, const ke_pod* pods, int64_t now, ke_pod_diagnosis* out,
                    int32_t words_per_pod, uint64_t* const* bits);
int device_schedule(Context* ctx, int32_t n_pods, const ke_pod* pods, int64_t now, int32_t* chosen, int32_t* score);
int device_rsv_result(Context* ctx, int32_t* out4);
int device_rsv_gate(const Context* ctx);
int device_refresh(Context* ctx, int64_t now, bool defer);
int device_ds_views(Context* ctx, const ke_pod& pod, int64_t now, const std::vector<DsView>& views,
                    std::vector<DsViewOut>& out);
int device_rsv_views(Context* ctx, const ke_pod& pod, int64_t now, const std::vector<RsvView>& views,
                     std::vector<RsvViewOut>& out);
int device_numa_views(Context* ctx, const ke_pod& pod, int64_t now, const std::vector<NumaRsvView>& views,
                      std::vector<NumaRsvOut>& out);
int device_quota_sync(Context* ctx);
int device_debug_rows(Context* ctx, int32_t n, Row* out);
int device_set_profiling(Context* ctx, int32_t every);
int device_set_pipeline(Context* ctx, int32_t on);
int device_replay_phases(Context* ctx, int which, double* cyc8);
int device_check_records(Context* ctx, int64_t now, int64_t* bad);
// (weak: a host-only build of this file, without ke_kernels.hip, links without it -- there is no device copy to check)
int device_spread_groups_check(Context* ctx, int64_t* bad) __attribute__((weak));
int device_spread_domains_check(Context* ctx, int64_t* bad) __attribute__((weak));
int device_devices_check(Context* ctx, int64_t* bad) __attribute__((weak));
int device_preempt(Context* ctx, int32_t n_pods, const ke_pod* pods, const PreemptPod* pre, int64_t now, ke_preemption* out,
                   int32_t victims_cap, int64_t* victim_uids, int32_t words_per_pod, uint64_t* candidates)
    __attribute__((weak));
int device_bench_eval(Context* ctx, int32_t n_pods, const ke_pod* pods, int64_t now, int32_t iters, double* avg_ms);
int device_comm_unique_id(uint8_t* id);
int device_shard_init(Context* ctx, int rank, int world, const uint8_t* id);
int device_shard_init_host(Context* ctx, int rank, int world, ke_host_collective fn, void* user);
int device_shard_range(Context* ctx, int* lo, int* hi);
bool device_sharded(const Context* ctx);
}  // namespace ke

using namespace ke;

// KOORDEVAL_RSV_FUSE=0: every reservation-matched pod is a segment of its own (the fused path's A/B)
static const bool kFuseMatched = [] {
  const char* e = std::getenv("KOORDEVAL_RSV_FUSE");
  return !e || std::atoi(e) != 0;
}();

// A ke_schedule_submit call: its device work in flight (`fin` set), or completed with its outputs kept until
// ke_schedule_wait collects them.
struct AsyncCall {
  int64_t ticket = 0;
  int32_t n = 0;
  const ke_pod* pods = nullptr;  // the caller's array (valid until its ke_schedule_wait)
  int64_t now = 0;
  bool device = false;  // enqueued by ke_schedule_submit (its release records are set when it is collected)
  DevFinish fin;
  int rc = KE_OK;
  std::string msg;
  std::vector<int32_t> chosen, score;
  // its release records: a copy of the Context's taken when it completes and restored when ke_schedule_wait collects
  // it, so a wait on an earlier ticket never pairs that call's nodes with a later call's cpusets / NUMA amounts /
  // device minors
  CallRecords rec;
};

struct ke_ctx {
  Context c;
  std::deque<AsyncCall> async;  // submitted, not yet collected (ticket order)
  int64_t next_ticket = 1;
};

// A submitted call's completion (in submission order): waits for its device work, takes its outputs and statistics,
// and queues its host mirror (the deferred LoadAware assign / NodeInfo.Requested of its placed pods).
static void async_finish(ke_ctx* ctx, AsyncCall& a) {
  if (!a.fin) return;
  DevFinish f = std::move(a.fin);
  a.fin = nullptr;
  a.chosen.assign((size_t)a.n, -1);
  a.score.assign((size_t)a.n, 0);
  a.rc = f(a.chosen.data(), a.score.data());
  if (a.rc) {
    a.msg = last_error_cstr();
    return;
  }
  Context& c = ctx->c;
  // the completion wrote this call's device / cpuset / VF / NUMA records into the Context; a plain queue assumes
  // no reservation and no quota
  c.last.resv.clear();
  c.last.set_pods(a.n, a.chosen.data(), a.pods, false, c.resv_gen);
  a.rec = c.last;
  const int32_t off = c.cfg.global_node_offset;
  const int64_t base = c.pending_base;  // the completion copied the pods there
  c.pending.reserve(c.pending.size() + (size_t)a.n);
  for (int32_t i = 0; i < a.n; i++) {
    const int32_t node = a.chosen[(size_t)i] - off;
    if (a.chosen[(size_t)i] < 0 || node < 0 || node >= c.n_nodes) continue;
    c.pending.push_back({node, a.now, base + i});
  }
}

// Every call in flight completes (an entry point that reads or changes the state the submitted calls work on).
static void async_drain(ke_ctx* ctx) {
  for (AsyncCall& a : ctx->async) async_finish(ctx, a);
  mirror_join(ctx->c);
}

static int check_node(ke_ctx* ctx, int32_t node) {
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  if (node < 0 || node >= ctx->c.cfg.node_capacity) return fail(KE_ERR_NOT_FOUND, "node index out of range");
  return KE_OK;
}

static int check_pods(const ke_pod* pods, int32_t n, const Context* c = nullptr, bool matched_ok = false) {
  if (n < 0 || (n > 0 && !pods)) return fail(KE_ERR_INVALID, "pods");
  for (int32_t p = 0; p < n; p++) {
    int rc = validate_pod(pods[p]);
    if (rc) return rc;
    const uint8_t rm = pods[p].reservation_matched;
    if (rm > KE_RSV_IGNORED) return fail(KE_ERR_INVALID, "ke_pod.reservation_matched");
    if (rm != KE_RSV_NONE && !matched_ok)
      return fail(KE_ERR_UNSUPPORTED, "a pod matching / ignoring reservations outside ke_schedule");
    if (c) rc = validate_pod_hints(*c, pods[p]);
    else if (pods[p].device_hint) rc = fail(KE_ERR_INVALID, "ke_pod.device_hint without a context");
    if (rc) return rc;
    if (c && c->cfg.fit.filter)  // NodeResourcesFit's Filter checks every requested scalar: it must have a slot
      for (int e = 0; e < pods[p].n_xres; e++) {
        const int32_t id = pods[p].xres_id[e];
        bool known = id == KE_XRES_CPU || id == KE_XRES_MEMORY || pods[p].xres_value[e] == 0;
        for (int q = 0; q < c->cfg.fit.n_scalars && !known; q++) known = c->cfg.fit.scalars[q] == id;
        if (!known) return fail(KE_ERR_UNSUPPORTED, "a pod requesting a scalar resource outside ke_fit_args.scalars");
      }
  }
  return KE_OK;
}

static int require_device(ke_ctx* ctx) {
  if (!ctx->c.dev) return fail(KE_ERR_NO_DEVICE, "evaluation needs the gfx950 device; this context has none");
  return KE_OK;
}

// A pod with its own NUMA topology policy switches the NUMA path on for every node (DeviceShare pods on
// NUMA-policy nodes take part in the topology manager's Admit as a second hint provider).
static int check_numa_deviceshare(ke_ctx* ctx, const ke_pod* pods, int32_t n) {
  for (int32_t p = 0; p < n; p++)
    if (pods[p].numa_topology_policy != KE_NUMA_POLICY_NONE) ctx->c.numa_enabled = true;
  return KE_OK;
}

// A pod that may bind CPUs (a cpuset pod, or any cpu request while a node forces CPU binding) reads the
// CPU SoA during evaluation: make sure it exists.
// The pods' DevPod records are staged for upload_pods (built once per call).
static int check_cpuset(ke_ctx* ctx, const ke_pod* pods, int32_t n) {
  Context& c = ctx->c;
  c.staged.resize((size_t)n);
  c.staged_src = pods;
  for (int32_t p = 0; p < n; p++) {
    c.staged[p] = make_dev_pod(c.cfg, pods[p], pod_hints(c, pods[p]), &c.tmpl);
    const uint32_t f = c.staged[p].flags;
    if ((f & PF_CPUSET) || (c.n_bind_nodes > 0 && pods[p].requests[KE_RES_CPU] > 0)) c.cpu_enabled = true;
  }
  return KE_OK;
}

// ke_pod_reservations lists of a ke_schedule call (consumed by it): shape, and the KE_RSV_MATCHED pods the
// nominated-reservation path supports.  Every refusal of that path is raised here, before the
// call schedules any pod: a refusal after earlier segments ran would leave their Reserves applied.
static int check_matches(Context& c, const ke_pod* pods, int32_t n) {
  const bool staged = !c.match_off.empty();
  if (staged && (int32_t)c.match_off.size() != n + 1)
    return fail(KE_ERR_INVALID, "ke_pod_reservations lists for a different number of pods");
  for (int32_t p = 0; p < n; p++) {
    const int32_t cnt = staged ? c.match_off[(size_t)p + 1] - c.match_off[(size_t)p] : 0;
    const uint8_t rm = pods[p].reservation_matched;
    if (rm != KE_RSV_MATCHED && rm != KE_RSV_AFFINITY) {
      if (cnt) return fail(KE_ERR_INVALID, "reservations listed for a pod that is not KE_RSV_MATCHED / AFFINITY");
      if (rm == KE_RSV_IGNORED) {
        const int rc = resv_ignore_check(c, pods[p], c.staged[(size_t)p].flags);
        if (rc) return rc;
      }
      continue;
    }
    if (!staged) return fail(KE_ERR_INVALID, "a KE_RSV_MATCHED / AFFINITY pod without ke_pod_reservations");
    const uint32_t f = c.staged[(size_t)p].flags;
    // (the Reservation plugin reads the pod's requests by name: every name other than cpu / memory through its
    // ke_pod.xres entry -- batch / mid resources and device resources included -- so a requested name without a
    // resource id is refused)
    if (pods[p].has_other_requests > 1 || pods[p].has_unsupported_device_requests)
      return fail(KE_ERR_UNSUPPORTED, "a pod matching reservations with unnamed resources");
    // a DeviceShare pod allocates from its matched reservations' devices (resv_ds_views) -- not with device hints /
    // joint allocation, nor in NUMA hints (a pod with a NUMA policy, or a NUMA-policy node, beside a matched
    // reservation holding devices)
    if ((f & (PF_DS | PF_DS_HINT)) && !c.resv_holds.empty())
      for (int32_t j = c.match_off[(size_t)p]; j < c.match_off[(size_t)p + 1]; j++) {
        const int32_t r = c.match_ids[(size_t)j];
        if (r < 0 || r >= (int32_t)c.resv.size() || !resv_usable(c.resv[(size_t)r]) ||
            !(c.resv_holds[(size_t)r] & KE_RSV_HOLDS_DEVICES))
          continue;
        if ((f & PF_DS_HINT) || pods[p].numa_topology_policy != KE_NUMA_POLICY_NONE ||
            c.nodes[(size_t)c.resv[(size_t)r].node].node.numa_topology_policy != KE_NUMA_POLICY_NONE)
          return fail(KE_ERR_UNSUPPORTED, "a DeviceShare pod with device hints or NUMA hints matching a reservation "
                                          "that holds devices");
      }
    // under a NUMA policy (the pod's or the node's) a matched reservation holding NUMA resources or CPUs enters the
    // hints through its allocate-from-reservation trials (k_numa_views) for a pod without device requests -- one
    // binding CPUs too (whole CPUs, not under a required FullPCPUs policy: preferredCPUs taken first may split cores,
    // which the per-view counts do not see); a DeviceShare pod's joint hints there are not restated, nor more than
    // NV_MAX such reservations of the pod on one node
    if (!c.resv_holds.empty()) {
      const bool binds = (f & PF_CPUSET) || (c.n_bind_nodes > 0 && pods[p].requests[KE_RES_CPU] > 0);
      const bool dev = (f & (PF_DS | PF_DS_HINT)) != 0;
      std::vector<std::pair<int32_t, int32_t>> per_node;
      for (int32_t j = c.match_off[(size_t)p]; j < c.match_off[(size_t)p + 1]; j++) {
        const int32_t r = c.match_ids[(size_t)j];
        if (r < 0 || r >= (int32_t)c.resv.size() || !resv_usable(c.resv[(size_t)r]) ||
            !(c.resv_holds[(size_t)r] & (KE_RSV_HOLDS_NUMA | KE_RSV_HOLDS_CPUSET)))
          continue;
        const int32_t node = c.resv[(size_t)r].node;
        const bool pol = pods[p].numa_topology_policy != KE_NUMA_POLICY_NONE ||
                         c.nodes[(size_t)node].node.numa_topology_policy != KE_NUMA_POLICY_NONE;
        const int preq = pf_cpu_required(f);
        const bool full_req = preq == XB_FULL || (preq == XB_NONE && c.nodes[(size_t)node].node.cpu_bind_policy ==
                                                                         KE_NODE_CPU_BIND_FULL_PCPUS_ONLY);
        if (pol && (dev || (binds && (!(f & PF_CPU_INT) || full_req))))
          return fail(KE_ERR_UNSUPPORTED, "a pod requesting devices, fractional CPUs or a required FullPCPUs binding "
                                          "under a NUMA topology policy matching a reservation that holds NUMA "
                                          "resources or CPUs");
        bool seen = false;
        for (auto& e : per_node)
          if (e.first == node) seen = true, e.second++;
        if (!seen) per_node.emplace_back(node, 1);
      }
      for (auto& e : per_node)
        if (e.second > NV_MAX)
          return fail(KE_ERR_UNSUPPORTED, "more matched reservations holding NUMA resources / CPUs on a node than "
                                          "NV_MAX");
    }
    const int rc = resv_check(c, c.match_ids.data() + c.match_off[(size_t)p], cnt);
    if (rc) return rc;
  }
  return KE_OK;
}

// a ke_last_* view of one device-made kind of the last call's records
template <class Kind, class T>
static int last_flat(ke_ctx* ctx, int32_t n, T* out, Kind CallRecords::*kind, const char* what) {
  if (!ctx || n < 0 || (n > 0 && !out)) return fail(KE_ERR_INVALID, what);
  (ctx->c.last.*kind).flat(n, out);
  return KE_OK;
}

// The staged ke_pod_reservations lists belong to the ke_schedule / ke_schedule_submit call that follows them, refused
// or not: the entry point holds one of these, and the lists are consumed when it returns.
struct StagedMatches {
  Context& c;
  ~StagedMatches() { c.match_off.clear(), c.match_ids.clear(); }
};

// One segment of a ke_schedule call (ke_segments.h): prepare -> schedule -> finish -> mirror -> refresh_quota.  It knows
// what it has done to the reservation state so far (`ignoring`, `held`) and undoes exactly that when it is left without
// resv_finish having assumed the pod: every error exit of the call is a plain return.  (A device failure leaves the
// context's state undefined, KE_ERR_DEVICE: rebuild it; a reservation's capacity still does not stay visible.)
struct SegmentRun {
  Context& c;
  const ke_pod* pods;
  int32_t n_pods;
  int64_t now;
  int32_t *chosen, *score, *assumed;
  const uint8_t* cls;  // PodClass bits per pod
  const Segment seg;
  int32_t len = seg.s1 - seg.s0;  // pods of the segment's record: with the fused pod once it has placed
  bool fuse = false;              // the pod after the segment runs last in the segment's call
  bool ignoring = false;          // resv_ignore_begin ran
  const ke_pod* held = nullptr;   // the matched pod whose views / restore the reservation state carries
  ~SegmentRun() {
    release();
    if (ignoring) resv_ignore_end(c);
  }
  const int32_t* ids(int32_t p) const { return c.match_ids.data() + c.match_off[(size_t)p]; }
  int32_t n_ids(int32_t p) const { return c.match_off[(size_t)p + 1] - c.match_off[(size_t)p]; }
  // the held pod's views' rows, nomination and restore back to what every other pod sees
  void release() {
    if (!held) return;
    for (const DsView& v : c.ds_views) resv_node_restore(c, v.node);
    for (const NumaRsvView& v : c.numa_views) resv_node_restore(c, v.node);
    int32_t none = 0;
    resv_finish(c, -1, *held, &none);
    held = nullptr;
  }
  // ---- the view sequences: trials on the current state, each in the order its plugins' restores need --------------
  template <class Fn, class V, class O>
  int trials(Fn device_views, const ke_pod& pod, const std::vector<V>& views, std::vector<O>& out) {
    return views.empty() ? KE_OK : device_views(&c, pod, now, views, out);
  }
  // a binding pod's cpuset and Score on the nomination / the Filter's affinity (NUMA policies)
  int cpuset_pass(const ke_pod& pod) {
    const int rc = trials(device_rsv_views, pod, c.numa_cs_views, c.numa_cs_out);
    if (!rc && !c.numa_cs_views.empty()) resv_numa_cs_apply(c);
    return rc;
  }
  // an ignored pod: its allocate-ignoring-reservation trials and NUMA hints, then DeviceShare's ignore / own views
  int ignored_views(const ke_pod& pod) {
    flush_mirror(c);
    resv_ignore_views(c, pod);
    int rc = trials(device_rsv_views, pod, c.rsv_views, c.rsv_view_out);
    if (!rc) rc = trials(device_numa_views, pod, c.numa_views, c.numa_view_out);
    if (!rc) resv_ds_views(c, pod, nullptr, 0), rc = trials(device_ds_views, pod, c.ds_views, c.ds_view_out);
    if (rc) return rc;
    resv_ignore_ovr(c);
    return cpuset_pass(pod);
  }
  // a matched pod: its allocate-from-reservation trials, DeviceShare's on the rows with its matched restore, then
  // NodeNUMAResource's hints over the trials; the nomination last
  int matched_views(int32_t p) {
    const ke_pod& pod = *(held = &pods[p]);
    resv_views(c, pod, ids(p), n_ids(p));
    int rc = trials(device_rsv_views, pod, c.rsv_views, c.rsv_view_out);
    if (!rc) resv_ds_views(c, pod, ids(p), n_ids(p)), rc = trials(device_ds_views, pod, c.ds_views, c.ds_view_out);
    if (!rc) resv_numa_views(c, pod, ids(p), n_ids(p)), rc = trials(device_numa_views, pod, c.numa_views, c.numa_view_out);
    if (!rc) rc = resv_prepare(c, pod, ids(p), n_ids(p), pod.reservation_matched == KE_RSV_AFFINITY);
    return rc ? rc : cpuset_pass(pod);
  }
  // the pod after a plain segment ("fused"): its nomination and rows are taken now, on the state before
  // the segment, when it needs no view and no allocate-from-reservation decision; else it stays a segment of its own
  int try_fuse(int32_t p) {
    if (int rc = device_refresh(&c, now, false)) return rc;  // the segment's rows (no host wait)
    held = &pods[p];
    resv_views(c, pods[p], ids(p), n_ids(p));
    fuse = c.rsv_views.empty();
    if (fuse) resv_ds_views(c, pods[p], ids(p), n_ids(p)), fuse = c.ds_views.empty();
    if (fuse) resv_numa_views(c, pods[p], ids(p), n_ids(p)), fuse = c.numa_views.empty();
    if (int rc = fuse ? resv_prepare(c, pods[p], ids(p), n_ids(p), false) : KE_OK) return rc;
    fuse = fuse && c.rsv_ovr.empty() && c.numa_cs_views.empty();
    if (!fuse) release();
    return KE_OK;
  }

  int prepare() {
    mirror_join(c);  // (the previous segment's host mirror thread: this one reads the node state)
    if (seg.ign) resv_ignore_begin(c), ignoring = true;
    if (seg.ign && seg.alone) return ignored_views(pods[seg.s0]);
    if (seg.matched()) return matched_views(seg.s0);
    const int32_t p = seg.s1;  // (matched, not ignoring: PC_ALONE alone)
    if (kFuseMatched && p < n_pods &&
        may_fuse(seg, (cls[p] & (PC_ALONE | PC_IGNORED)) == PC_ALONE && pods[p].reservation_matched == KE_RSV_MATCHED,
                 !(c.staged[(size_t)p].flags & (PF_CPUSET | PF_DS | PF_DS_HINT)), !c.quotas.empty(), device_sharded(&c)))
      return try_fuse(p);
    return KE_OK;
  }

  int schedule() {
    c.rsv_fused = fuse;
    c.att.gangs = c.gang_words.empty() ? nullptr : c.gang_words.data() + seg.s0;  // the segment's gang words
    const int rc = device_schedule(&c, len + fuse, pods + seg.s0, now, chosen + seg.s0, score ? score + seg.s0 : nullptr);
    c.rsv_fused = false;
    return rc;
  }
  // The Reservation plugin's outcome of the held pod, at position `pos` of the segment's record: k_rsv_pick's winner is
  // the placement, its ScoreReservation joins the score, the pod is assumed with the cpuset / NUMA amounts / minors it got
  int matched_outcome(int32_t pos) {
    const int32_t p = seg.s0 + pos;
    const int32_t local = chosen[p] < 0 ? -1 : chosen[p] - c.cfg.global_node_offset;
    int32_t pick[4] = {local, 0, 0, -1};  // no usable matched reservation: no Reservation score
    if (int rc = !c.rsv_pairs.empty() || c.rsv_affinity ? device_rsv_result(&c, pick) : KE_OK) return rc;
    if (local >= 0 && local != pick[0]) return fail(KE_ERR_DEVICE, "k_rsv_pick winner differs from the placement");
    if (local >= 0 && score) score[p] = (int32_t)((int64_t)score[p] + c.cfg.weight_reservation * (int64_t)pick[1]);
    resv_finish(c, local, *held, &assumed[p], c.last.cpuset(pos), c.last.numa(pos), c.last.dev(pos));
    held = nullptr;
    return KE_OK;
  }

  int finish() {
    if (ignoring) resv_ignore_end(c), ignoring = false;
    if (fuse && device_rsv_gate(&c)) {
      // k_rsv_check: a plain pod took a node of the fused pod's reservations and the pod placed nothing; its nomination
      // and rows are undone and it runs next as a segment of its own (the call's per-pod outputs: the segment's only)
      release();
      chosen[seg.s1] = -1;
      c.last.truncate((size_t)len);
      if (c.last_pod_lat.size() > (size_t)len) c.last_pod_lat.resize((size_t)len);
      if (!c.last_batch_ms.empty()) c.last_batch_ms.pop_back();
      c.last_rsv_fused_gated++;
      fuse = false;
    } else if (fuse) {
      if (int rc = matched_outcome(len)) return rc;
      c.last_rsv_fused++, len++;
    }
    return seg.matched() ? matched_outcome(0) : KE_OK;
  }

  // Host mirror of the Reserves the device already applied to its rows: keep the object state (assign cache,
  // NodeInfo.Requested) in step so later re-derivations include these pods.
  void mirror() {
    const auto tp = std::chrono::steady_clock::now();
    c.pending.reserve(c.pending.size() + (size_t)len);
    const int64_t base = c.pending_base;  // device_schedule copied the segment's pods there during its wait
    for (int32_t i = 0; i < len; i++) {
      const int32_t p = seg.s0 + i, node = chosen[p] - c.cfg.global_node_offset;
      if (chosen[p] < 0 || node < 0 || node >= c.n_nodes) continue;
      // LoadAware assign + NodeInfo.Requested: deferred (flush_mirror), the device rows carry them
      c.pending.push_back({node, now, base + i});
      // the allocations (read back only when the call's batches could make them): only a pod that has one touches the node
      const uint64_t dev = c.last.dev(i);
      const int64_t* numa = c.last.numa(i);
      const uint64_t* cs = c.last.cpuset(i);
      const bool cpus = cs && (cs[0] | cs[1] | cs[2] | cs[3]);
      if (!dev && !numa && !cpus) continue;
      mirror_join(c);  // (the earlier calls' mirror may still be running on its thread)
      NodeState& ns = c.nodes[node];
      const bool was_dirty = ns.dirty;
      if (dev) host_ds_reserve(c.cfg, ns, make_dev_pod(c.cfg, pods[p], pod_hints(c, pods[p]), &c.tmpl), dev, c.last.vf(i));
      if (numa) host_numa_reserve(ns, numa);
      ns.dirty = was_dirty;  // the device rows already carry these Reserves
      // cpuset Reserve: the CPU table and the zones' NUMA status (not patched on the device: re-derived from this mirror)
      if (cpus) host_cpuset_reserve(ns, make_dev_pod(c.cfg, pods[p]), cs);
    }
    c.host_ms[7] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp).count();
  }

  // ElasticQuota: a Reserve into the system / default quota (limit_is_max) with runtime quota on shrinks
  // totalResourceExceptSystemAndDefaultUsed (group_quota_manager.go:268-271, 127-151) and every later pod sees limits
  // refreshed from it: the host takes the device's used, shrinks the total by the pod's masked request and recomputes
  int refresh_quota() {
    const ke_pod& pod = pods[seg.s1 - 1];
    if (!seg.barrier || chosen[seg.s1 - 1] < 0) return KE_OK;
    if (int rc = device_quota_sync(&c)) return rc;
    const ke_quota& q = c.quotas[(size_t)pod.quota - 1];
    c.qargs.total[0] -= q.has_max[0] ? pod.requests[KE_RES_CPU] : 0;
    c.qargs.total[1] -= q.has_max[1] ? pod.requests[KE_RES_MEMORY] : 0;
    const int rc = quota_compute_limits(c.qargs, c.quotas, c.qlimit, c.qlimit_has);
    if (!rc) c.quota_dirty = true;
    return rc;
  }
};

extern "C" {

int ke_abi_version(void) { return KE_ABI_VERSION; }
int ke_abi_struct_sizes(int32_t* sizes, int32_t n) {
  const int32_t all[] = {(int32_t)sizeof(ke_config),       (int32_t)sizeof(ke_node),
                         (int32_t)sizeof(ke_node_metric),  (int32_t)sizeof(ke_pod_metric),
                         (int32_t)sizeof(ke_aggregated_usage), (int32_t)sizeof(ke_pod),
                         (int32_t)sizeof(ke_resource_map), (int32_t)sizeof(ke_loadaware_args),
                         (int32_t)sizeof(ke_numa_args), (int32_t)sizeof(ke_deviceshare_args),
                         (int32_t)sizeof(ke_device),       (int32_t)sizeof(ke_numa_zone),
                         (int32_t)sizeof(ke_cpu),          (int32_t)sizeof(ke_quota_args),
                         (int32_t)sizeof(ke_quota),        (int32_t)sizeof(ke_gpu_partition),
                         (int32_t)sizeof(ke_ext_args),     (int32_t)sizeof(ke_node_resource),
                         (int32_t)sizeof(ke_pod_allocation), (int32_t)sizeof(ke_pod_device_hints),
                         (int32_t)sizeof(ke_gpu_template),   (int32_t)sizeof(ke_reservation),
                         (int32_t)sizeof(ke_reservation_alloc), (int32_t)sizeof(ke_reservation_resource),
                         (int32_t)sizeof(ke_pod_diagnosis)};
  const int32_t m = (int32_t)(sizeof(all) / sizeof(all[0]));
  for (int32_t i = 0; i < n && i < m; i++) sizes[i] = all[i];
  return m;
}
const char* ke_last_error(void) { return last_error_cstr(); }
int ke_device_available(void) { return device_available(); }
int ke_row_bytes(void) { return ROW_BYTES; }
int ke_pod_record_bytes(void) { return (int)sizeof(DevPod); }

int ke_create(const ke_config* cfg, ke_ctx** out) {
  if (!cfg || !out) return fail(KE_ERR_INVALID, "null argument");
  *out = nullptr;
  int rc = validate_config(*cfg);
  if (rc) return rc;
  ke_ctx* ctx = new (std::nothrow) ke_ctx();
  if (!ctx) return fail(KE_ERR_INVALID, "out of memory");
  Context& c = ctx->c;
  c.cfg = *cfg;
  c.nodes.resize((size_t)cfg->node_capacity);
  c.residents.nodes.resize((size_t)cfg->node_capacity);
  for (int32_t i = 0; i < cfg->node_capacity; i++) c.nodes[(size_t)i].dirty.bind(i, &c.dirty_list);
  KArgs& k = c.kargs_template;
  const ke_loadaware_args& a = cfg->loadaware;
  k.exp_s = a.node_metric_expiration_seconds;
  uint32_t f = 0;
  if (a.filter_expired_node_metrics) f |= AF_FILTER_EXPIRED;
  if (a.enable_schedule_when_node_metrics_expired) f |= AF_ENABLE_WHEN_EXPIRED;
  if (a.node_metric_expiration_seconds != KE_ABSENT) f |= AF_EXP_PRESENT;
  if (cfg->numa.strategy == KE_STRATEGY_MOST_ALLOCATED) f |= AF_NUMA_MOST;
  if (cfg->deviceshare.strategy == KE_STRATEGY_MOST_ALLOCATED) f |= AF_DS_MOST;
  if (cfg->deviceshare.disable_numa_alignment) f |= AF_DS_NO_NUMA;
  if (cfg->numa.numa_strategy == KE_STRATEGY_MOST_ALLOCATED) f |= AF_NUMA_HINT_MOST;
  k.flags = f;
  k.wsum_la = k.wsum_numa = 0;
  for (int r = 0; r < KE_NRES; r++) {
    k.w_la[r] = a.resource_weights[r] == KE_ABSENT ? 0 : (int32_t)a.resource_weights[r];
    k.w_numa[r] = cfg->numa.weights[r] == KE_ABSENT ? 0 : (int32_t)cfg->numa.weights[r];
    k.wsum_la += k.w_la[r];
    k.wsum_numa += k.w_numa[r];
  }
  k.wp_la = (int32_t)cfg->weight_loadaware;
  k.wp_numa = (int32_t)cfg->weight_numa;
  k.wp_ds = (int32_t)cfg->weight_deviceshare;
  for (int i = 0; i < 4; i++)
    k.w_ds[i] = cfg->deviceshare.weights[i] == KE_ABSENT ? -1 : (int32_t)cfg->deviceshare.weights[i];
  // NodeResourcesFitPlus / ScarceResourceAvoidance: their Score joins every evaluation path (eval_pair,
  // lite_total, and the fast replay's fast_total from the node's ext words)
  // and NodeResourcesFit: ext slots (ext_slots: FitPlus resources first, then Fit's resources and scalars)
  const ke_ext_args& x = cfg->ext;
  const ke_fit_args& fa = cfg->fit;
  k.wp_fp = (int32_t)x.weight_fitplus;
  k.wp_sra = (int32_t)x.weight_sra;
  k.wp_fit = (int32_t)fa.weight;
  k.sra_mask = x.sra_resources;
  int32_t ids[2 * NUM_XS + KE_MAX_FITPLUS];
  k.xs_n = ext_slots(*cfg, ids);
  k.fp_mask = k.fp_most = k.fit_mask = k.fit_scalar = 0;
  for (int q = 0; q < NUM_XS; q++) {
    k.xs_id[q] = q < k.xs_n ? ids[q] : 0;
    k.fp_w[q] = k.fit_w[q] = 0;
  }
  for (int q = 0; q < x.n_fitplus; q++) {  // FitPlus resource q is slot q
    k.fp_mask |= 1u << q;
    k.fp_w[q] = x.fitplus[q].weight;
    if (x.fitplus[q].type == KE_STRATEGY_MOST_ALLOCATED) k.fp_most |= 1u << q;
  }
  for (int q = 0; q < k.xs_n; q++) {
    for (int r = 0; r < fa.n_resources; r++)
      if (fa.resources[r].id == k.xs_id[q]) k.fit_mask |= 1u << q, k.fit_w[q] = fa.resources[r].weight;
    for (int r = 0; r < fa.n_scalars; r++)
      if (fa.scalars[r] == k.xs_id[q]) k.fit_scalar |= 1u << q;
  }
  if (fa.filter) k.flags |= AF_FIT_FILTER;
  if (fa.strategy == KE_STRATEGY_MOST_ALLOCATED) k.flags |= AF_FIT_MOST;
  if (x.weight_fitplus > 0 || x.weight_sra > 0 || fa.weight > 0 || fa.filter) {
    k.flags |= AF_EXT;
    c.ext_enabled = true;
  }
  if (device_available()) {
    rc = device_create(&c);
    if (rc) {
      device_destroy(&c);
      delete ctx;
      return rc;
    }
  }
  *out = ctx;
  return KE_OK;
}

void ke_destroy(ke_ctx* ctx) {
  if (!ctx) return;
  async_drain(ctx);
  device_destroy(&ctx->c);
  delete ctx;
}

int32_t ke_num_nodes(ke_ctx* ctx) { return ctx ? ctx->c.n_nodes : 0; }

int ke_node_resources_set(ke_ctx* ctx, int32_t node, int32_t n, const ke_node_resource* res) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  rc = validate_node_resources(n, res);
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  ns.xres.assign(res, res + n);
  ns.dirty = true;
  ctx->c.n_nodes = std::max(ctx->c.n_nodes, node + 1);
  return KE_OK;
}

int ke_node_resources_get(ke_ctx* ctx, int32_t node, int32_t cap, ke_node_resource* res, int32_t* n) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  if (!n || cap < 0 || (cap > 0 && !res)) return fail(KE_ERR_INVALID, "ke_node_resources_get arguments");
  const NodeState& ns = ctx->c.nodes[node];
  *n = (int32_t)ns.xres.size();
  for (int32_t e = 0; e < cap && e < *n; e++) res[e] = ns.xres[e];
  return KE_OK;
}

int ke_debug_rsv_fused(ke_ctx* ctx, int64_t* out2) {
  if (!ctx || !out2) return fail(KE_ERR_INVALID, "ke_debug_rsv_fused arguments");
  out2[0] = ctx->c.last_rsv_fused;
  out2[1] = ctx->c.last_rsv_fused_gated;
  return KE_OK;
}

int ke_debug_ds_cuts(ke_ctx* ctx, int32_t* cuts) {
  if (!ctx || !cuts) return fail(KE_ERR_INVALID, "ke_debug_ds_cuts arguments");
  *cuts = ctx->c.last_ds_cuts;
  return KE_OK;
}

int ke_node_upsert(ke_ctx* ctx, int32_t node, const ke_node* n) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  if (!n) return fail(KE_ERR_INVALID, "null node");
  rc = validate_node(*n);
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  if (ns.valid) {
    ctx->c.n_bind_nodes -= ns.node.cpu_bind_policy != KE_NODE_CPU_BIND_NONE;
    ctx->c.n_policy_nodes -= ns.node.numa_topology_policy != KE_NUMA_POLICY_NONE;
  }
  ns.valid = true;
  ns.known = true;
  ns.node = *n;
  ns.dirty = true;
  ctx->c.n_bind_nodes += n->cpu_bind_policy != KE_NODE_CPU_BIND_NONE;
  ctx->c.n_policy_nodes += n->numa_topology_policy != KE_NUMA_POLICY_NONE;
  if (n->numa_topology_policy != KE_NUMA_POLICY_NONE) ctx->c.numa_enabled = true;
  ctx->c.n_nodes = std::max(ctx->c.n_nodes, node + 1);
  return KE_OK;
}

int ke_node_delete(ke_ctx* ctx, int32_t node) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);  // pending Reserves on it first: the object state stays (koord_eval.h)
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  resident_drop(ctx->c.residents, node);  // its resident pods go with it (ke_preempt.h)
  if (!ns.valid) return KE_OK;
  ctx->c.n_bind_nodes -= ns.node.cpu_bind_policy != KE_NODE_CPU_BIND_NONE;
  ctx->c.n_policy_nodes -= ns.node.numa_topology_policy != KE_NUMA_POLICY_NONE;
  ns.valid = false;  // derive_row: no NF_VALID -> every Filter path fails the node
  ns.dirty = true;
  return KE_OK;
}

int ke_node_topology_delete(ke_ctx* ctx, int32_t node) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  // the NodeAllocation stays (resource_manager.go keeps nodeAllocations[node] until the Node itself goes)
  if (!ns.cpus.empty()) ns.kept_cpus = ns.cpus;
  if (!ns.zones.empty()) ns.kept_zones = ns.zones;
  ns.zones.clear();
  ns.cpus.clear();
  ns.cpu_max_ref = 1;
  ns.node.cpuset_allocated_cpus = 0;        // GetAvailableCPUs without a CPU topology: no allocated CPUs
  ns.node.nrt_cpu_amplification_ratio = -2;  // no NRT ratio map
  ns.node.cpu_topology_invalid = 0;
  ns.dirty = true;
  return KE_OK;
}

int ke_nodes_load(ke_ctx* ctx, int32_t n, const ke_node* nodes) {
  if (ctx) async_drain(ctx);
  if (!ctx || n < 0 || (n > 0 && !nodes)) return fail(KE_ERR_INVALID, "ke_nodes_load arguments");
  if (ctx) flush_mirror(ctx->c);
  if (n > ctx->c.cfg.node_capacity) return fail(KE_ERR_INVALID, "more nodes than node_capacity");
  for (int32_t i = 0; i < n; i++) {
    int rc = ke_node_upsert(ctx, i, &nodes[i]);
    if (rc) return rc;
  }
  return KE_OK;
}

int ke_node_devices_set(ke_ctx* ctx, int32_t node, int32_t n, const ke_device* devices) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  rc = validate_devices(n, devices);
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  ns.has_dev_cache = true;
  ns.devs.assign(devices, devices + n);
  rc = intern_device_labels(ctx->c, ns);
  if (rc) return rc;
  ns.dirty = true;
  ctx->c.ds_enabled = true;
  return KE_OK;
}

int ke_node_device_flags(ke_ctx* ctx, int32_t node, int32_t secondary_well_planned, int32_t gpu_model_key) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  const int id = intern_model_key(ctx->c, gpu_model_key);
  if (id < 0) return id;
  NodeState& ns = ctx->c.nodes[node];
  ns.secondary_well_planned = secondary_well_planned != 0;
  ns.gpu_model_id = id;
  ns.dirty = true;
  return KE_OK;
}

int ke_set_pod_device_hints(ke_ctx* ctx, int32_t n, const ke_pod_device_hints* hints) {
  if (ctx) async_drain(ctx);
  if (!ctx || n < 0 || (n > 0 && !hints)) return fail(KE_ERR_INVALID, "ke_set_pod_device_hints arguments");
  ctx->c.hints.assign(hints, hints + n);
  return KE_OK;
}

int ke_gpu_templates_load(ke_ctx* ctx, int32_t n, const ke_gpu_template* templates) {
  if (ctx) async_drain(ctx);
  if (!ctx || n < 0 || (n > 0 && !templates)) return fail(KE_ERR_INVALID, "ke_gpu_templates_load arguments");
  for (int32_t i = 0; i < n; i++) {
    const int id = intern_model_key(ctx->c, templates[i].model_key);
    if (id < 0) return id;
  }
  ctx->c.tmpl.assign(templates, templates + n);
  return KE_OK;
}

int ke_reservations_load(ke_ctx* ctx, int32_t n, const ke_reservation* reservations) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  flush_mirror(ctx->c);
  return load_reservations(ctx->c, n, reservations);
}

int ke_reservations_load_ex(ke_ctx* ctx, int32_t n, const ke_reservation* reservations,
                            const ke_reservation_alloc* allocs) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  flush_mirror(ctx->c);
  return load_reservations(ctx->c, n, reservations, allocs);
}

int ke_reservations_load_full(ke_ctx* ctx, int32_t n, const ke_reservation* reservations,
                              const ke_reservation_alloc* allocs, const int32_t* res_offsets,
                              const ke_reservation_resource* res) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  if (!res_offsets) return fail(KE_ERR_INVALID, "ke_reservations_load_full: res_offsets");
  flush_mirror(ctx->c);
  return load_reservations(ctx->c, n, reservations, allocs, res_offsets, res);
}

int ke_reservation_resources_get(ke_ctx* ctx, int32_t r, int32_t cap, ke_reservation_resource* out, int32_t* n) {
  if (ctx) async_drain(ctx);
  if (!ctx || !n || cap < 0 || (cap > 0 && !out) || r < 0 || r >= (int32_t)ctx->c.resv.size())
    return fail(KE_ERR_INVALID, "ke_reservation_resources_get arguments");
  const auto& e = (size_t)r < ctx->c.resv_res.size() ? ctx->c.resv_res[(size_t)r] : std::vector<ke_reservation_resource>{};
  *n = (int32_t)e.size();
  for (int32_t i = 0; i < cap && i < *n; i++) out[i] = e[(size_t)i];
  return KE_OK;
}

int ke_reservation_allocs_get(ke_ctx* ctx, int32_t n, ke_reservation_alloc* out) {
  if (ctx) async_drain(ctx);
  if (!ctx || n < 0 || (n > 0 && !out) || n > (int32_t)ctx->c.resv.size())
    return fail(KE_ERR_INVALID, "ke_reservation_allocs_get arguments");
  for (int32_t i = 0; i < n; i++)
    out[i] = ctx->c.resv_alloc.empty() ? ke_reservation_alloc{} : ctx->c.resv_alloc[(size_t)i];
  return KE_OK;
}

int32_t ke_reservations_generation(ke_ctx* ctx) { return ctx ? ctx->c.resv_gen : 0; }

int ke_reservations_get(ke_ctx* ctx, int32_t n, ke_reservation* out) {
  if (ctx) async_drain(ctx);
  if (!ctx || n < 0 || (n > 0 && !out) || n > (int32_t)ctx->c.resv.size()) return fail(KE_ERR_INVALID, "ke_reservations_get arguments");
  std::copy(ctx->c.resv.begin(), ctx->c.resv.begin() + n, out);
  return KE_OK;
}

int ke_pod_reservations(ke_ctx* ctx, int32_t n_pods, const int32_t* offsets, const int32_t* ids) {
  if (ctx) async_drain(ctx);
  if (!ctx || n_pods < 0 || !offsets) return fail(KE_ERR_INVALID, "ke_pod_reservations arguments");
  Context& c = ctx->c;
  if (offsets[0] != 0) return fail(KE_ERR_INVALID, "ke_pod_reservations offsets[0] != 0");
  for (int32_t p = 0; p < n_pods; p++)
    if (offsets[p + 1] < offsets[p]) return fail(KE_ERR_INVALID, "ke_pod_reservations offsets decrease");
  if (offsets[n_pods] > 0 && !ids) return fail(KE_ERR_INVALID, "ke_pod_reservations ids");
  for (int32_t j = 0; j < offsets[n_pods]; j++)
    if (ids[j] < 0 || ids[j] >= (int32_t)c.resv.size()) return fail(KE_ERR_NOT_FOUND, "ke_pod_reservations: reservation index");
  c.match_off.assign(offsets, offsets + n_pods + 1);
  c.match_ids.assign(ids, ids + offsets[n_pods]);
  return KE_OK;
}

// ---- per-pod node eligibility sets (include/koord_eval.h) ----
int ke_node_sets_load(ke_ctx* ctx, int32_t n_sets, int32_t words_per_set, const uint64_t* bits) {
  if (ctx) async_drain(ctx);
  if (!ctx || n_sets < 0 || words_per_set < 0) return fail(KE_ERR_INVALID, "ke_node_sets_load arguments");
  if (n_sets > KE_MAX_NODE_SETS) return fail(KE_ERR_INVALID, "ke_node_sets_load: more than KE_MAX_NODE_SETS sets");
  if (words_per_set > (1 << 20)) return fail(KE_ERR_INVALID, "ke_node_sets_load: words_per_set");
  if (n_sets > 0 && !bits) return fail(KE_ERR_INVALID, "ke_node_sets_load: bits");
  Context& c = ctx->c;
  c.ns_n = n_sets;
  c.ns_wps = n_sets > 0 ? words_per_set : 0;
  c.ns_bits.assign(bits, bits + (n_sets > 0 ? (size_t)n_sets * (size_t)words_per_set : 0));
  c.ns_dirty = true;
  c.ns_dirty_words.clear();
  return KE_OK;
}

int ke_node_set_bits(ke_ctx* ctx, int32_t node, int32_t n_sets, const uint8_t* member) {
  if (ctx) async_drain(ctx);
  if (!ctx || (n_sets > 0 && !member)) return fail(KE_ERR_INVALID, "ke_node_set_bits arguments");
  Context& c = ctx->c;
  if (n_sets != c.ns_n) return fail(KE_ERR_INVALID, "ke_node_set_bits: n_sets differs from the loaded table's");
  if (node < 0 || (int64_t)node >= 64 * (int64_t)c.ns_wps)
    return fail(KE_ERR_NOT_FOUND, "ke_node_set_bits: node index beyond the table's words_per_set");
  const uint64_t bit = 1ull << (node & 63);
  for (int32_t s = 0; s < n_sets; s++) {
    uint64_t& w = c.ns_bits[(size_t)s * (size_t)c.ns_wps + (size_t)(node >> 6)];
    w = member[s] ? (w | bit) : (w & ~bit);
  }
  if (!c.ns_dirty) c.ns_dirty_words.push_back(node >> 6);  // (the next call with a non-zero id uploads the column)
  return KE_OK;
}

// The four per-pod id stagings (ke_pod_node_sets, ke_pod_node_scores, ke_pod_spread_groups, ke_pod_spread_domains): ids
// in 0..the loaded table's rows, staged for the next call
static int stage_pod_ids(ke_ctx* ctx, int32_t n_pods, const int32_t* ids, const char* fn, const char* outside,
                         int32_t Context::*limit, AttachSlot<int32_t> Context::*slot) {
  if (!ctx || n_pods < 0 || (n_pods > 0 && !ids)) return fail(KE_ERR_INVALID, std::string(fn) + " arguments");
  Context& c = ctx->c;
  for (int32_t p = 0; p < n_pods; p++)
    if (ids[p] < 0 || ids[p] > c.*limit) return fail(KE_ERR_INVALID, std::string(fn) + ": " + outside);
  (c.*slot).stage(ids, n_pods);
  return KE_OK;
}

int ke_pod_node_sets(ke_ctx* ctx, int32_t n_pods, const int32_t* set_ids) {
  return stage_pod_ids(ctx, n_pods, set_ids, "ke_pod_node_sets", "set id outside 0..n_sets", &Context::ns_n, &Context::pod_sets);
}

// ---- per-pod node score offsets (include/koord_eval.h): the node sets' lifecycle ----
// The highest table entry the packed key's 10-bit score field leaves room for: total + 1 <= 1023 with every
// Score plugin of the context at 100 (validate_config's sum).
static int32_t node_score_cap(const ke_config& cfg) {
  return MAX_TOTAL_SCORE - 100 * (cfg.weight_loadaware + cfg.weight_numa + cfg.weight_deviceshare + cfg.ext.weight_fitplus +
                                  cfg.ext.weight_sra + cfg.fit.weight);
}
static int node_score_above_cap(const char* fn, int32_t cap) {
  return fail(KE_ERR_UNSUPPORTED, std::string(fn) + ": an entry above " + std::to_string(cap) +
                                      " = 1022 - 100 * (sum of the Score plugin weights): total + 1 must fit the key's 10 bits");
}

int ke_node_scores_load(ke_ctx* ctx, int32_t n_tables, int32_t n_nodes, const uint16_t* scores) {
  if (ctx) async_drain(ctx);
  if (!ctx || n_tables < 0 || n_nodes < 0) return fail(KE_ERR_INVALID, "ke_node_scores_load arguments");
  if (n_tables > KE_MAX_NODE_SCORE_TABLES)
    return fail(KE_ERR_INVALID, "ke_node_scores_load: more than KE_MAX_NODE_SCORE_TABLES tables");
  if (n_nodes > MAX_SHARD_NODES) return fail(KE_ERR_INVALID, "ke_node_scores_load: n_nodes");
  if (n_tables > 0 && !scores) return fail(KE_ERR_INVALID, "ke_node_scores_load: scores");
  Context& c = ctx->c;
  const size_t n = n_tables > 0 ? (size_t)n_tables * (size_t)n_nodes : 0;
  const int32_t cap = node_score_cap(c.cfg);
  for (size_t q = 0; q < n; q++)
    if ((int32_t)scores[q] > cap) return node_score_above_cap("ke_node_scores_load", cap);
  c.nsc_n = n_tables;
  c.nsc_nodes = n_tables > 0 ? n_nodes : 0;
  c.nsc_vals.assign(scores, scores + n);
  c.nsc_dirty = true;
  c.nsc_dirty_nodes.clear();
  return KE_OK;
}

int ke_node_scores_set(ke_ctx* ctx, int32_t node, int32_t n_tables, const uint16_t* column) {
  if (ctx) async_drain(ctx);
  if (!ctx || (n_tables > 0 && !column)) return fail(KE_ERR_INVALID, "ke_node_scores_set arguments");
  Context& c = ctx->c;
  if (n_tables != c.nsc_n) return fail(KE_ERR_INVALID, "ke_node_scores_set: n_tables differs from the loaded table's");
  if (node < 0 || node >= c.nsc_nodes) return fail(KE_ERR_NOT_FOUND, "ke_node_scores_set: node index beyond the table's n_nodes");
  const int32_t cap = node_score_cap(c.cfg);
  for (int32_t t = 0; t < n_tables; t++)
    if ((int32_t)column[t] > cap) return node_score_above_cap("ke_node_scores_set", cap);
  for (int32_t t = 0; t < n_tables; t++) c.nsc_vals[(size_t)t * (size_t)c.nsc_nodes + (size_t)node] = column[t];
  if (!c.nsc_dirty) c.nsc_dirty_nodes.push_back(node);  // (the next call with a non-zero id uploads the column)
  return KE_OK;
}

int ke_pod_node_scores(ke_ctx* ctx, int32_t n_pods, const int32_t* table_ids) {
  return stage_pod_ids(ctx, n_pods, table_ids, "ke_pod_node_scores", "table id outside 0..n_tables", &Context::nsc_n,
                       &Context::pod_scores);
}

// ---- spread groups (include/koord_eval.h): the node sets' lifecycle ----
int ke_spread_groups_load(ke_ctx* ctx, int32_t n_groups, int32_t n_nodes, const uint16_t* counts,
                          const uint16_t* max_per_node) {
  if (ctx) async_drain(ctx);
  if (!ctx || n_groups < 0 || n_nodes < 0) return fail(KE_ERR_INVALID, "ke_spread_groups_load arguments");
  if (n_groups > KE_MAX_SPREAD_GROUPS) return fail(KE_ERR_INVALID, "ke_spread_groups_load: more than KE_MAX_SPREAD_GROUPS groups");
  if (n_nodes > MAX_SHARD_NODES) return fail(KE_ERR_INVALID, "ke_spread_groups_load: n_nodes");
  if (n_groups > 0 && !max_per_node) return fail(KE_ERR_INVALID, "ke_spread_groups_load: max_per_node");
  for (int32_t g = 0; g < n_groups; g++)
    if (max_per_node[g] < 1) return fail(KE_ERR_INVALID, "ke_spread_groups_load: a cap below 1");
  Context& c = ctx->c;
  c.sg_n = n_groups;
  c.sg_nodes = n_groups > 0 ? n_nodes : 0;
  // (a Reserve may land on any node of the context: the host copy has an entry for each, zero beyond n_nodes)
  c.sg_stride = n_groups > 0 ? std::max<int64_t>(n_nodes, c.cfg.node_capacity) : 0;
  c.sg_cnt.assign((size_t)n_groups * (size_t)c.sg_stride, 0);
  if (counts)
    for (int32_t g = 0; g < n_groups; g++)
      std::copy(counts + (size_t)g * (size_t)n_nodes, counts + (size_t)(g + 1) * (size_t)n_nodes,
                c.sg_cnt.begin() + (int64_t)g * c.sg_stride);
  c.sg_cap.assign(max_per_node, max_per_node + n_groups);
  c.sg_dirty = true;
  c.sg_dirty_cells.clear();
  return KE_OK;
}

int ke_spread_group_add(ke_ctx* ctx, int32_t group, int32_t node, int32_t delta) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "ke_spread_group_add arguments");
  Context& c = ctx->c;
  if (group < 1 || group > c.sg_n) return fail(KE_ERR_NOT_FOUND, "ke_spread_group_add: group outside 1..n_groups");
  if (node < 0 || (int64_t)node >= c.sg_stride) return fail(KE_ERR_NOT_FOUND, "ke_spread_group_add: node index beyond the table");
  uint16_t& v = c.sg_cnt[(size_t)(group - 1) * (size_t)c.sg_stride + (size_t)node];
  const int64_t nv = std::max<int64_t>((int64_t)v + delta, 0);
  if (nv > 65535) return fail(KE_ERR_INVALID, "ke_spread_group_add: the count would pass 65535");
  v = (uint16_t)nv;
  if (!c.sg_dirty) c.sg_dirty_cells.push_back({group, node});  // (the next call with a non-zero id uploads the entry)
  return KE_OK;
}

int ke_spread_groups_get(ke_ctx* ctx, int32_t group, int32_t n_nodes, uint16_t* counts) {
  if (ctx) async_drain(ctx);
  if (!ctx || n_nodes < 0 || (n_nodes > 0 && !counts)) return fail(KE_ERR_INVALID, "ke_spread_groups_get arguments");
  const Context& c = ctx->c;
  if (group < 1 || group > c.sg_n) return fail(KE_ERR_NOT_FOUND, "ke_spread_groups_get: group outside 1..n_groups");
  const uint16_t* row = c.sg_cnt.data() + (size_t)(group - 1) * (size_t)c.sg_stride;
  for (int32_t i = 0; i < n_nodes; i++) counts[i] = (int64_t)i < c.sg_stride ? row[i] : (uint16_t)0;
  return KE_OK;
}

int ke_pod_spread_groups(ke_ctx* ctx, int32_t n_pods, const int32_t* group_ids) {
  return stage_pod_ids(ctx, n_pods, group_ids, "ke_pod_spread_groups", "group id outside 0..n_groups", &Context::sg_n,
                       &Context::pod_groups);
}

// ---- spread domains (include/koord_eval.h): the spread groups' lifecycle ----
int ke_spread_domains_load(ke_ctx* ctx, int32_t n_maps, int32_t n_nodes, const uint16_t* node_domain, int32_t n_groups,
                           const int32_t* group_map, const uint64_t* domains, const int32_t* max_skew,
                           const int32_t* min_domains, const uint32_t* counts) {
  if (ctx) async_drain(ctx);
  if (!ctx || n_maps < 0 || n_nodes < 0 || n_groups < 0) return fail(KE_ERR_INVALID, "ke_spread_domains_load arguments");
  if (n_groups > KE_MAX_SPREAD_DOMAIN_GROUPS)
    return fail(KE_ERR_INVALID, "ke_spread_domains_load: more than KE_MAX_SPREAD_DOMAIN_GROUPS groups");
  if (n_groups > 0 && n_maps > KE_MAX_SPREAD_DOMAIN_MAPS)
    return fail(KE_ERR_INVALID, "ke_spread_domains_load: more than KE_MAX_SPREAD_DOMAIN_MAPS maps");
  if (n_nodes > MAX_SHARD_NODES) return fail(KE_ERR_INVALID, "ke_spread_domains_load: n_nodes");
  Context& c = ctx->c;
  if (n_groups > 0) {
    if (n_maps < 1 || (n_nodes > 0 && !node_domain)) return fail(KE_ERR_INVALID, "ke_spread_domains_load: node_domain");
    if (!group_map || !domains || !max_skew) return fail(KE_ERR_INVALID, "ke_spread_domains_load: a group array is NULL");
    for (int64_t q = 0; q < (int64_t)n_maps * n_nodes; q++)
      if (node_domain[q] >= KE_MAX_SPREAD_DOMAINS && node_domain[q] != KE_DOMAIN_NONE)
        return fail(KE_ERR_INVALID, "ke_spread_domains_load: a domain id above 63");
    for (int32_t g = 0; g < n_groups; g++) {
      if (group_map[g] < 1 || group_map[g] > n_maps) return fail(KE_ERR_INVALID, "ke_spread_domains_load: a group's map outside 1..n_maps");
      if (domains[g] == 0) return fail(KE_ERR_INVALID, "ke_spread_domains_load: a group without a domain");
      if (max_skew[g] < 1) return fail(KE_ERR_INVALID, "ke_spread_domains_load: a max_skew below 1");
      if (min_domains && min_domains[g] < 0) return fail(KE_ERR_INVALID, "ke_spread_domains_load: a negative min_domains");
      for (int32_t d = 0; counts && d < KE_MAX_SPREAD_DOMAINS; d++)
        if (counts[(size_t)g * KE_MAX_SPREAD_DOMAINS + (size_t)d] > (uint32_t)INT32_MAX)
          return fail(KE_ERR_INVALID, "ke_spread_domains_load: a count above 2^31-1");
    }
  }
  c.sd_n = n_groups;
  c.sd_maps = n_groups > 0 ? n_maps : 0;
  // (a Reserve may land on any node of the context: the host copy has an entry for each, NONE beyond n_nodes)
  c.sd_stride = n_groups > 0 ? std::max<int64_t>(n_nodes, c.cfg.node_capacity) : 0;
  c.sd_map.assign((size_t)c.sd_maps * (size_t)c.sd_stride, (uint16_t)KE_DOMAIN_NONE);
  for (int32_t m = 0; m < c.sd_maps; m++)
    std::copy(node_domain + (size_t)m * (size_t)n_nodes, node_domain + (size_t)(m + 1) * (size_t)n_nodes,
              c.sd_map.begin() + (int64_t)m * c.sd_stride);
  c.sd_gmap.assign(group_map, group_map + n_groups);
  c.sd_dom.assign(domains, domains + n_groups);
  c.sd_skew.assign(max_skew, max_skew + n_groups);
  c.sd_mind.assign((size_t)n_groups, 0);
  if (min_domains) std::copy(min_domains, min_domains + n_groups, c.sd_mind.begin());
  c.sd_cnt.assign((size_t)n_groups * KE_MAX_SPREAD_DOMAINS, 0u);
  if (counts) std::copy(counts, counts + (size_t)n_groups * KE_MAX_SPREAD_DOMAINS, c.sd_cnt.begin());
  c.sd_dirty = true;
  c.sd_dirty_cells.clear();
  c.sd_dirty_nodes.clear();
  return KE_OK;
}

int ke_spread_domain_add(ke_ctx* ctx, int32_t group, int32_t domain, int32_t delta) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "ke_spread_domain_add arguments");
  Context& c = ctx->c;
  if (group < 1 || group > c.sd_n) return fail(KE_ERR_NOT_FOUND, "ke_spread_domain_add: group outside 1..n_groups");
  if (domain < 0 || domain >= KE_MAX_SPREAD_DOMAINS) return fail(KE_ERR_NOT_FOUND, "ke_spread_domain_add: domain outside 0..63");
  uint32_t& v = c.sd_cnt[(size_t)(group - 1) * KE_MAX_SPREAD_DOMAINS + (size_t)domain];
  const int64_t nv = std::max<int64_t>((int64_t)v + delta, 0);
  if (nv > INT32_MAX) return fail(KE_ERR_INVALID, "ke_spread_domain_add: the count would pass 2^31-1");
  v = (uint32_t)nv;
  if (!c.sd_dirty) c.sd_dirty_cells.push_back({group, domain});  // (the next call with a non-zero id uploads the entry)
  return KE_OK;
}

int ke_spread_domain_node_set(ke_ctx* ctx, int32_t map, int32_t node, int32_t domain) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "ke_spread_domain_node_set arguments");
  Context& c = ctx->c;
  if (map < 1 || map > c.sd_maps) return fail(KE_ERR_NOT_FOUND, "ke_spread_domain_node_set: map outside 1..n_maps");
  if (node < 0 || (int64_t)node >= c.sd_stride) return fail(KE_ERR_NOT_FOUND, "ke_spread_domain_node_set: node index beyond the maps");
  if ((domain < 0 || domain >= KE_MAX_SPREAD_DOMAINS) && domain != KE_DOMAIN_NONE)
    return fail(KE_ERR_INVALID, "ke_spread_domain_node_set: domain outside 0..63 and not KE_DOMAIN_NONE");
  c.sd_map[(size_t)(map - 1) * (size_t)c.sd_stride + (size_t)node] = (uint16_t)domain;
  if (!c.sd_dirty) c.sd_dirty_nodes.push_back({map, node});
  return KE_OK;
}

int ke_spread_domains_get(ke_ctx* ctx, int32_t group, uint32_t* counts64) {
  if (ctx) async_drain(ctx);
  if (!ctx || !counts64) return fail(KE_ERR_INVALID, "ke_spread_domains_get arguments");
  const Context& c = ctx->c;
  if (group < 1 || group > c.sd_n) return fail(KE_ERR_NOT_FOUND, "ke_spread_domains_get: group outside 1..n_groups");
  std::copy(c.sd_cnt.begin() + (int64_t)(group - 1) * KE_MAX_SPREAD_DOMAINS,
            c.sd_cnt.begin() + (int64_t)group * KE_MAX_SPREAD_DOMAINS, counts64);
  return KE_OK;
}

int ke_pod_spread_domains(ke_ctx* ctx, int32_t n_pods, const int32_t* group_ids) {
  return stage_pod_ids(ctx, n_pods, group_ids, "ke_pod_spread_domains", "group id outside 0..n_groups", &Context::sd_n,
                       &Context::pod_domains);
}

// ---- spread terms (include/koord_eval.h): ke_pod_spread_groups' rules, per-pod lists ----
static_assert(KE_MAX_POD_TERMS == POD_TERMS && KE_MAX_POD_MEMBERS == POD_MEMBERS && KE_TERM_ANTI == ST_ANTI &&
                  KE_TERM_AFFINITY == ST_AFFINITY && KE_TERM_PREFER_FEWER == ST_PREFER_FEWER &&
                  KE_TERM_PREFER_MORE == ST_PREFER_MORE && KE_MAX_SPREAD_GROUPS < (1 << 16),
              "the packed record");
// ke_pod_spread_terms and ke_pod_spread_domain_terms share the CSR checks and the packed record:
// `name` leads every message, `n_groups` is the table the groups are checked against, `max_kind` the last kind
// (KE_TERM_SKEW, param and weight 0, only over the spread domain table).
static int stage_term_lists(ke_ctx* ctx, int32_t n_pods, const int32_t* term_offsets, const int32_t* terms,
                            const int32_t* member_offsets, const int32_t* members, const char* name,
                            int32_t Context::*n_groups, int32_t max_kind, AttachSlot<PodTerms> Context::*slot) {
  auto bad = [name](const char* what) { return fail(KE_ERR_INVALID, std::string(name) + what); };
  if (!ctx || n_pods < 0 || !term_offsets || !member_offsets) return bad(" arguments");
  Context& c = ctx->c;
  const int32_t limit = c.*n_groups;
  if (term_offsets[0] != 0 || member_offsets[0] != 0) return bad(": offsets do not start at 0");
  for (int32_t p = 0; p < n_pods; p++) {
    if (term_offsets[p + 1] < term_offsets[p] || member_offsets[p + 1] < member_offsets[p])
      return bad(": offsets do not ascend");
    if (term_offsets[p + 1] - term_offsets[p] > KE_MAX_POD_TERMS)
      return bad(": more than KE_MAX_POD_TERMS terms for one pod");
    if (member_offsets[p + 1] - member_offsets[p] > KE_MAX_POD_MEMBERS)
      return bad(": more than KE_MAX_POD_MEMBERS members for one pod");
  }
  if ((term_offsets[n_pods] > 0 && !terms) || (member_offsets[n_pods] > 0 && !members))
    return bad(" arguments");
  std::vector<PodTerms> recs((size_t)n_pods, PodTerms{});
  for (int32_t p = 0; p < n_pods; p++) {
    PodTerms& r = recs[(size_t)p];
    for (int32_t q = term_offsets[p], t = 0; q < term_offsets[p + 1]; q++, t++) {
      const int32_t group = terms[4 * q], kind = terms[4 * q + 1], param = terms[4 * q + 2], weight = terms[4 * q + 3];
      if (group < 1 || group > limit) return bad(": a term's group outside 1..n_groups");
      if (kind < KE_TERM_ANTI || kind > max_kind) return bad(": unknown term kind");
      if (kind == KE_TERM_SKEW) {
        if (param != 0 || weight != 0) return bad(": KE_TERM_SKEW with a non-zero param or weight");
        r.tw[t] = (uint32_t)group | (uint32_t)kind << 16;
        continue;
      }
      if (param < 1 || param > 65535) return bad(": a param outside 1..65535");
      const bool score = kind == KE_TERM_PREFER_FEWER || kind == KE_TERM_PREFER_MORE;
      if (score ? (weight < 1 || weight > 100) : weight != 0)
        return bad(": a weight outside 1..100 (score terms) or not 0 (filter terms)");
      r.tw[t] = (uint32_t)group | (uint32_t)kind << 16 | (uint32_t)weight << 24;
      r.tp[t >> 1] |= (uint32_t)param << ((t & 1) * 16);
    }
    for (int32_t q = member_offsets[p], m = 0; q < member_offsets[p + 1]; q++, m++) {
      const int32_t group = members[q];
      if (group < 1 || group > limit) return bad(": a member outside 1..n_groups");
      for (int32_t u = member_offsets[p]; u < q; u++)
        if (members[u] == group) return bad(": a repeated member");
      r.mem[m >> 1] |= (uint32_t)group << ((m & 1) * 16);
    }
  }
  (c.*slot).stage(recs);
  return KE_OK;
}
int ke_pod_spread_terms(ke_ctx* ctx, int32_t n_pods, const int32_t* term_offsets, const int32_t* terms,
                        const int32_t* member_offsets, const int32_t* members) {
  return stage_term_lists(ctx, n_pods, term_offsets, terms, member_offsets, members, "ke_pod_spread_terms", &Context::sg_n,
                          KE_TERM_PREFER_MORE, &Context::pod_terms);
}
static_assert(KE_TERM_SKEW == ST_SKEW && KE_MAX_SPREAD_DOMAIN_GROUPS < (1 << 16), "the packed record");
int ke_pod_spread_domain_terms(ke_ctx* ctx, int32_t n_pods, const int32_t* term_offsets, const int32_t* terms,
                               const int32_t* member_offsets, const int32_t* members) {
  return stage_term_lists(ctx, n_pods, term_offsets, terms, member_offsets, members, "ke_pod_spread_domain_terms",
                          &Context::sd_n, KE_TERM_SKEW, &Context::pod_dterms);
}

// The ke_pod_node_sets, ke_pod_node_scores, ke_pod_spread_groups and ke_pod_spread_domains ids of this call, all
// consumed whether it goes on or not; Context::att names the ids of a kind when any of them is non-zero (the device
// entry points then run the node-set / score-offset / spread-group / spread-domain kernels).  Such a call is refused
// here, before any state changes, where those kernels are not built: node-sharded contexts, and for ke_schedule
// (`sched`) anything but a plain queue (ke_schedule_submit's sense, with device_async_ok's conditions).  The message
// names the sets when a set id is non-zero, else the scores when a table id is, else the spread groups, else the spread
// domains, else the spread terms.  ke_pod_spread_terms' lists go the same way: att.terms = the call's
// records when one of them is not empty; staged together with group ids they are KE_ERR_INVALID, and a pod whose score
// terms could push total + 1 out of the key's 10 bits is KE_ERR_UNSUPPORTED.  ke_pod_spread_domain_terms' lists (§4u)
// likewise: att.dterms; staged together with group ids or spread domain ids they are KE_ERR_INVALID, and their score
// terms count against the same cap, summed per pod with its §4t score terms.  `filter_only` (ke_diagnose): the call
// is checked as any other and then goes on without its score table ids, which do not filter.
// The id kinds, in the order of every check and of the message prefix:
enum { AK_SETS, AK_SCORES, AK_GROUPS, AK_DOMAINS, N_ID_KINDS };
static const struct {
  AttachSlot<int32_t> Context::*slot;
  int32_t Context::*limit;
  const int32_t* CallAttach::*view;
  const char *mismatch, *outside, *prefix;
} ID_KINDS[N_ID_KINDS] = {
    {&Context::pod_sets, &Context::ns_n, &CallAttach::sets, "the call's n_pods differs from the staged ke_pod_node_sets ids'",
     "a staged node set id is outside the table loaded since", "node sets: "},
    {&Context::pod_scores, &Context::nsc_n, &CallAttach::scores, "the call's n_pods differs from the staged ke_pod_node_scores ids'",
     "a staged node score table id is outside the table loaded since", "node scores: "},
    {&Context::pod_groups, &Context::sg_n, &CallAttach::groups, "the call's n_pods differs from the staged ke_pod_spread_groups ids'",
     "a staged spread group id is outside the table loaded since", "spread groups: "},
    {&Context::pod_domains, &Context::sd_n, &CallAttach::domains, "the call's n_pods differs from the staged ke_pod_spread_domains ids'",
     "a staged spread domain group id is outside the table loaded since", "spread domains: "},
};
static int take_node_sets(ke_ctx* ctx, int32_t n_pods, const ke_pod* pods, bool sched, bool filter_only = false) {
  Context& c = ctx->c;
  c.att.reset();
  if (!sched) c.pod_gangs.take(), c.gang_words.clear();  // (runs belong to a ke_schedule call: any other call drops them)
  if (!(c.pod_sets.on || c.pod_scores.on || c.pod_groups.on || c.pod_domains.on || c.pod_terms.on || c.pod_dterms.on))
    return KE_OK;
  bool on[N_ID_KINDS], any[N_ID_KINDS] = {false, false, false, false};
  for (int k = 0; k < N_ID_KINDS; k++) on[k] = (c.*ID_KINDS[k].slot).take();
  const bool terms_on = c.pod_terms.take();
  const bool dterms_on = c.pod_dterms.take();
  for (int k = 0; k < N_ID_KINDS; k++)
    if (on[k] && (int32_t)(c.*ID_KINDS[k].slot).call.size() != n_pods) return fail(KE_ERR_INVALID, ID_KINDS[k].mismatch);
  if (terms_on && (int32_t)c.pod_terms.call.size() != n_pods)
    return fail(KE_ERR_INVALID, "the call's n_pods differs from the staged ke_pod_spread_terms lists'");
  if (terms_on && on[AK_GROUPS])
    return fail(KE_ERR_INVALID, "a call with both ke_pod_spread_groups ids and ke_pod_spread_terms lists staged");
  if (dterms_on && (int32_t)c.pod_dterms.call.size() != n_pods)
    return fail(KE_ERR_INVALID, "the call's n_pods differs from the staged ke_pod_spread_domain_terms lists'");
  if (dterms_on && on[AK_GROUPS])
    return fail(KE_ERR_INVALID, "a call with both ke_pod_spread_groups ids and ke_pod_spread_domain_terms lists staged: "
                                "write group g as ke_pod_spread_terms {ANTI(g, cap)} + {g}");
  if (dterms_on && on[AK_DOMAINS])
    return fail(KE_ERR_INVALID, "a call with both ke_pod_spread_domains ids and ke_pod_spread_domain_terms lists staged: "
                                "write group g as {KE_TERM_SKEW(g)} + {g}");
  for (int k = 0; k < N_ID_KINDS; k++)
    for (int32_t id : (c.*ID_KINDS[k].slot).call) {
      if (id < 0 || id > c.*ID_KINDS[k].limit) return fail(KE_ERR_INVALID, ID_KINDS[k].outside);
      any[k] = any[k] || id != 0;
    }
  bool any_st = false;
  int32_t st_sum = 0;  // the largest bonus a pod's score terms can add
  for (const PodTerms& r : c.pod_terms.call) {
    int32_t sum = 0;
    for (int t = 0; t < POD_TERMS; t++) {
      if (st_group(r, t) > c.sg_n) return fail(KE_ERR_INVALID, "a staged spread term's group is outside the table loaded since");
      if (st_kind(r, t) >= ST_PREFER_FEWER) sum += st_weight(r, t) * (int32_t)st_param(r, t);
    }
    for (int m = 0; m < POD_MEMBERS; m++)
      if (st_member(r, m) > c.sg_n) return fail(KE_ERR_INVALID, "a staged spread member is outside the table loaded since");
    st_sum = std::max(st_sum, sum);
    c.att.listed.push_back(st_empty(r) ? 0 : 1);
    any_st = any_st || !st_empty(r);
  }
  // the domain term lists: over the spread domain table; a pod's score terms of both kinds add up against one cap
  bool any_dt = false;
  if (dterms_on) c.att.listed.resize((size_t)n_pods, 0);
  for (size_t p = 0; p < c.pod_dterms.call.size(); p++) {
    const PodTerms& r = c.pod_dterms.call[p];
    int32_t sum = 0;
    for (int t = 0; t < POD_TERMS; t++) {
      if (st_group(r, t) > c.sd_n) return fail(KE_ERR_INVALID, "a staged spread domain term's group is outside the table loaded since");
      if (st_kind(r, t) == ST_PREFER_FEWER || st_kind(r, t) == ST_PREFER_MORE) sum += st_weight(r, t) * (int32_t)st_param(r, t);
    }
    for (int m = 0; m < POD_MEMBERS; m++)
      if (st_member(r, m) > c.sd_n) return fail(KE_ERR_INVALID, "a staged spread domain member is outside the table loaded since");
    if (terms_on) {
      const PodTerms& q = c.pod_terms.call[p];
      for (int t = 0; t < POD_TERMS; t++)
        if (st_kind(q, t) >= ST_PREFER_FEWER) sum += st_weight(q, t) * (int32_t)st_param(q, t);
    }
    st_sum = std::max(st_sum, sum);
    if (!st_empty(r)) c.att.listed[p] = 1, any_dt = true;
  }
  const bool any_sc = any[AK_SCORES];
  // (the first kind present names a refusal)
  const char* prefix = any_st ? "spread terms: " : any_dt ? "spread domain terms: " : nullptr;
  for (int k = N_ID_KINDS - 1; k >= 0; k--)
    if (any[k]) prefix = ID_KINDS[k].prefix;
  if (!prefix) return KE_OK;
  int rc = check_pods(pods, n_pods, &c, sched);
  if (rc) return rc;
  auto no = [prefix](const char* what) { return fail(KE_ERR_UNSUPPORTED, std::string(prefix) + what); };
  if (c.cfg.global_node_offset != 0 || (c.dev && device_sharded(&c))) return no("a node-sharded context");
  if (sched) {
    if (!c.match_off.empty()) return no("a call with staged ke_pod_reservations lists");
    if (!c.quotas.empty()) return no("a context with an ElasticQuota tree");
    if (c.numa_enabled) return no("a context with NUMA topology policy state");
    if (c.n_bind_nodes > 0) return no("a context with CPU bind policy nodes");
    for (int32_t p = 0; p < n_pods; p++) {
      if (pods[p].reservation_matched != KE_RSV_NONE) return no("a reservation-matched / ignored / affinity pod in ke_schedule");
      if (pods[p].numa_topology_policy != KE_NUMA_POLICY_NONE) return no("a NUMA-policy pod in ke_schedule");
      if (pods[p].quota != 0) return no("an ElasticQuota pod in ke_schedule");
      const uint32_t f = make_dev_pod(c.cfg, pods[p], pod_hints(c, pods[p]), &c.tmpl).flags;
      if (f & (PF_DS | PF_DS_HINT)) return no("a DeviceShare pod in ke_schedule");
      if (f & PF_CPUSET) return no("a cpuset pod in ke_schedule");
    }
  }
  if (any_st || any_dt) {
    // the key holds total + 1 in 10 bits: the plugins' total, the largest table entry the call can add and the
    // largest bonus of a pod must fit together
    int32_t cap = node_score_cap(c.cfg);
    if (any_sc && !c.nsc_vals.empty()) cap -= (int32_t)*std::max_element(c.nsc_vals.begin(), c.nsc_vals.end());
    if (st_sum > cap)
      return fail(KE_ERR_UNSUPPORTED, std::string(any_dt ? "spread domain terms: " : "spread terms: ") + "a pod's score terms can add " + std::to_string(st_sum) + ", above the cap " +
                                          std::to_string(cap) + " = 1022 - 100 * (sum of the Score plugin weights)" +
                                          (any_sc ? " - the largest score table entry" : "") +
                                          ": total + 1 must fit the key's 10 bits");
    if (any_st) c.att.terms = c.pod_terms.call.data();
    if (any_dt) c.att.dterms = c.pod_dterms.call.data();
  }
  for (int k = 0; k < N_ID_KINDS; k++)
    if (any[k] && !(filter_only && k == AK_SCORES)) c.att.*ID_KINDS[k].view = (c.*ID_KINDS[k].slot).call.data();
  c.att.n_pods = n_pods;
  return KE_OK;
}

// ---- gang runs (include/koord_eval.h; the run logic is ke_gang.h's) ----
int ke_pod_gangs(ke_ctx* ctx, int32_t n_pods, int32_t n_runs, const ke_gang_run* runs) {
  if (!ctx) return fail(KE_ERR_INVALID, "ke_pod_gangs arguments");
  const char* why = "";
  const int rc = gang_validate(n_pods, n_runs, runs, &why);
  if (rc) return fail(rc, why);
  ctx->c.pod_gangs.stage(runs, n_runs);
  ctx->c.pod_gangs_n = n_pods;
  return KE_OK;
}
int ke_abi_gang_struct_sizes(int32_t* sizes, int32_t n) {
  const int32_t all[] = {(int32_t)sizeof(ke_gang_run)};
  const int32_t m = (int32_t)(sizeof(all) / sizeof(all[0]));
  for (int32_t i = 0; i < n && i < m; i++) sizes[i] = all[i];
  return m;
}
int ke_last_gang_status(ke_ctx* ctx, int32_t n, int32_t* status, int32_t* tried_node) {
  if (!ctx || n < 0 || (n > 0 && (!status || !tried_node))) return fail(KE_ERR_INVALID, "ke_last_gang_status arguments");
  const CallRecords& r = ctx->c.last;
  for (int32_t p = 0; p < n; p++) {
    status[p] = r.gang_status.at(p) ? *r.gang_status.at(p) : KE_GANG_NONE;
    tried_node[p] = r.gang_tried.at(p) ? *r.gang_tried.at(p) : -1;
  }
  return KE_OK;
}
int ke_debug_gangs(ke_ctx* ctx, int64_t* out4) {
  if (!ctx || !out4) return fail(KE_ERR_INVALID, "ke_debug_gangs arguments");
  for (int i = 0; i < 4; i++) out4[i] = ctx->c.last.gang_counts[i];
  return KE_OK;
}
int ke_set_gang_devices(ke_ctx* ctx, int32_t on) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  ctx->c.gang_devices = on != 0;
  return KE_OK;
}
int ke_debug_gang_devices(ke_ctx* ctx, int64_t* out4) {
  if (!ctx || !out4) return fail(KE_ERR_INVALID, "ke_debug_gang_devices arguments");
  for (int i = 0; i < 4; i++) out4[i] = ctx->c.last.gang_dev_counts[i];
  return KE_OK;
}

// The staged runs of this ke_schedule / ke_schedule_submit call (behind take_node_sets, which reset Context::att),
// consumed whether the call goes on or not.  Every refusal of a gang call is raised here, before any state changes and
// without a device; a call with at least one run goes on with Context::gang_words, its pods' gang words.
static int take_gangs(ke_ctx* ctx, int32_t n_pods, const ke_pod* pods) {
  Context& c = ctx->c;
  c.gang_words.clear();
  if (!c.pod_gangs.take()) return KE_OK;
  const std::vector<ke_gang_run>& runs = c.pod_gangs.call;
  if (c.pod_gangs_n != n_pods) return fail(KE_ERR_INVALID, "the call's n_pods differs from the staged ke_pod_gangs runs'");
  if (runs.empty()) return KE_OK;
  int rc = check_pods(pods, n_pods, &c, true);
  if (rc) return rc;
  auto no = [](const char* what) { return fail(KE_ERR_UNSUPPORTED, std::string("gangs: ") + what); };
  if (c.att.groups || c.att.domains || c.att.terms || c.att.dterms)
    return no("a call with spread group / spread domain ids or term lists");
  if ((c.att.sets || c.att.scores) && !c.quotas.empty()) return no("an ElasticQuota tree together with node sets or score tables");
  if (c.cfg.global_node_offset != 0 || (c.dev && device_sharded(&c))) return no("a node-sharded context");
  if (!c.match_off.empty()) return no("a call with staged ke_pod_reservations lists");
  if (c.numa_enabled || c.n_policy_nodes > 0) return no("a context with NUMA topology policy state");
  if (c.n_bind_nodes > 0) return no("a context with CPU bind policy nodes");
  const bool barriers = !c.quotas.empty() && c.qargs.enable_runtime_quota;
  for (const ke_gang_run& r : runs) {
    if (r.count > c.cfg.pod_batch) return no("a run longer than ke_config.pod_batch");
    for (int32_t p = r.first; p < r.first + r.count; p++) {
      if (pods[p].reservation_matched != KE_RSV_NONE) return no("a reservation-matched / ignored / affinity member");
      if (pods[p].numa_topology_policy != KE_NUMA_POLICY_NONE) return no("a NUMA-policy member");
      if (pods[p].quota < 0 || pods[p].quota > (int32_t)c.quotas.size())
        return fail(KE_ERR_INVALID, "ke_pod.quota outside the loaded ElasticQuota tree");
      if (barriers && pods[p].quota > 0 && c.quotas[(size_t)pods[p].quota - 1].limit_is_max)
        return no("a member whose quota Reserve refreshes the runtime quota (a segment barrier)");
      const uint32_t f = make_dev_pod(c.cfg, pods[p], pod_hints(c, pods[p]), &c.tmpl).flags;
      if (f & PF_DS_HINT) return no("a member with device hints");
      if ((f & PF_DS) && c.gang_devices) {
        if (!c.quotas.empty()) return no("a DeviceShare member together with an ElasticQuota tree");
        if (c.n_nodes <= 0) return no("a DeviceShare member in a context without nodes");
      } else if (f & PF_DS) {
        return no("a DeviceShare member");
      }
      if (f & PF_CPUSET) return no("a cpuset member");
    }
  }
  c.gang_words = gang_words(n_pods, (int32_t)runs.size(), runs.data());
  c.att.gangs = c.gang_words.data();  // (ke_schedule: each segment's own words, SegmentRun::schedule)
  return KE_OK;
}

int ke_node_info_requested(ke_ctx* ctx, int32_t node, int64_t* requested, int64_t* non_zero) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (rc) return rc;
  if (!requested || !non_zero) return fail(KE_ERR_INVALID, "ke_node_info_requested outputs");
  flush_mirror(ctx->c);
  const NodeState& ns = ctx->c.nodes[node];
  for (int k = 0; k < KE_NRES; k++) {
    requested[k] = ns.node.requested[k] + ns.rv_req[k];
    non_zero[k] = KE_ABSENT;  // NonZeroRequested is known from the node's ke_node_resources_set rows
    for (const ke_node_resource& r : ns.xres)
      if (r.id == k) non_zero[k] = xres_requested(ns, r);
  }
  return KE_OK;
}

int ke_node_gpu_partitions(ke_ctx* ctx, int32_t node, int32_t has_table, int32_t honor, int32_t n,
                           const ke_gpu_partition* partitions) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  if (n > 0 && !has_table) return fail(KE_ERR_INVALID, "partitions without a table");
  int id = -1;
  if (has_table) {
    id = ptable_intern(ctx->c, n, partitions);
    if (id < 0) return id;
  }
  NodeState& ns = ctx->c.nodes[node];
  ns.ptable = id;
  ns.gpu_honor = honor != 0;
  ns.dirty = true;
  return KE_OK;
}

int ke_node_devices_delete(ke_ctx* ctx, int32_t node) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  ns.has_dev_cache = false;
  ns.devs.clear();
  ns.ptable = -1;
  ns.gpu_honor = false;
  ns.dirty = true;
  return KE_OK;
}

int ke_node_numa_set(ke_ctx* ctx, int32_t node, int32_t n, const ke_numa_zone* zones) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  rc = validate_zones(n, zones);
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  ns.zones.assign(zones, zones + n);
  for (ke_numa_zone& z : ns.zones) normalize_zone(z);
  bool bare = true;  // an NRT without the resource manager's allocation: the parked one comes back
  for (const ke_numa_zone& z : ns.zones)
    bare = bare && !z.has_allocated && !z.single_pods && !z.shared_pods && !z.cpuset_cpus;
  if (bare)
    for (ke_numa_zone& z : ns.zones)
      for (const ke_numa_zone& k : ns.kept_zones)
        if (k.id == z.id) {
          z.has_allocated = k.has_allocated;
          for (int r = 0; r < KE_NRES; r++) z.allocated[r] = k.allocated[r];
          z.cpuset_cpus = k.cpuset_cpus;
          z.single_pods = k.single_pods;
          z.shared_pods = k.shared_pods;
          z.numa_status = zone_status(z);
        }
  if (n > 0) ns.kept_zones.clear();
  ns.dirty = true;
  ctx->c.numa_enabled = true;
  return KE_OK;
}

int ke_node_cpus_set(ke_ctx* ctx, int32_t node, int32_t n, const ke_cpu* cpus, int32_t max_ref_count) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  rc = validate_cpus(n, cpus, max_ref_count);
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  ns.cpus.assign(cpus, cpus + n);
  ns.cpu_max_ref = n > 0 ? max_ref_count : 1;
  bool bare = true;  // a topology without allocatedCPUs: the parked NodeAllocation comes back by CPU id
  for (const ke_cpu& c : ns.cpus) bare = bare && c.ref_count == 0;
  if (bare)
    for (ke_cpu& c : ns.cpus)
      for (const ke_cpu& k : ns.kept_cpus)
        if (k.cpu_id == c.cpu_id) c.ref_count = k.ref_count, c.exclusive = k.exclusive;
  if (n > 0) ns.kept_cpus.clear();
  ns.dirty = true;
  if (n > 0) ctx->c.cpu_enabled = true;
  return KE_OK;
}

int ke_quotas_load(ke_ctx* ctx, const ke_quota_args* args, const ke_quota* quotas, int32_t n) {
  if (ctx) async_drain(ctx);
  if (!ctx || !args || n < 0 || n > KE_MAX_QUOTAS || (n > 0 && !quotas)) return fail(KE_ERR_INVALID, "ke_quotas_load arguments");
  if (args->n_hook_plugins) return fail(KE_ERR_UNSUPPORTED, "ElasticQuotaArgs.HookPlugins are not supported");
  if (args->enable_guarantee_usage) return fail(KE_ERR_UNSUPPORTED, "ElasticQuotaGuaranteeUsage is not supported");
  for (int r = 0; r < KE_NRES; r++)
    if (args->total[r] < 0) return fail(KE_ERR_INVALID, "ke_quota_args.total must be >= 0");
  std::vector<ke_quota> q(quotas, quotas + n);
  for (const ke_quota& x : q)
    for (int r = 0; r < KE_NRES; r++)
      if (x.max[r] < 0 || x.min[r] < 0 || x.shared_weight[r] < 0 || x.self_request[r] < 0 || x.used[r] < 0 ||
          x.non_preemptible_used[r] < 0)
        return fail(KE_ERR_INVALID, "ke_quota values must be >= 0");
  std::vector<int64_t> lim;
  std::vector<uint8_t> has;
  const int rc = quota_compute_limits(*args, q, lim, has);
  if (rc) return rc;
  Context& c = ctx->c;
  c.qargs = *args;
  c.quotas.swap(q);
  c.qlimit.swap(lim);
  c.qlimit_has.swap(has);
  c.quota_dirty = true;
  c.quota_on_device = false;
  return KE_OK;
}

int ke_quota_state(ke_ctx* ctx, int32_t q, int64_t* limit, uint8_t* limit_has, int64_t* used, int64_t* np_used) {
  if (ctx) async_drain(ctx);
  if (!ctx || q < 0 || q >= (int32_t)ctx->c.quotas.size()) return fail(KE_ERR_NOT_FOUND, "ke_quota_state: no such quota");
  const int rc = device_quota_sync(&ctx->c);
  if (rc) return rc;
  const ke_quota& x = ctx->c.quotas[q];
  for (int r = 0; r < KE_NRES; r++) {
    if (limit) limit[r] = ctx->c.qlimit[(size_t)q * KE_NRES + r];
    if (limit_has) limit_has[r] = ctx->c.qlimit_has[(size_t)q * KE_NRES + r];
    if (used) used[r] = x.used[r];
    if (np_used) np_used[r] = x.non_preemptible_used[r];
  }
  return KE_OK;
}

int ke_last_cpusets(ke_ctx* ctx, int32_t n, uint64_t* out) { return last_flat(ctx, n, out, &CallRecords::cpusets, "ke_last_cpusets arguments"); }

int ke_last_numa_allocations(ke_ctx* ctx, int32_t n, int64_t* out) { return last_flat(ctx, n, out, &CallRecords::numas, "ke_last_numa_allocations arguments"); }

int ke_last_device_allocations(ke_ctx* ctx, int32_t n, uint64_t* minors) { return last_flat(ctx, n, minors, &CallRecords::devs, "ke_last_device_allocations arguments"); }

int ke_node_set_requested(ke_ctx* ctx, int32_t node, int64_t milli_cpu, int64_t memory) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  ns.node.requested[KE_RES_CPU] = milli_cpu;
  ns.node.requested[KE_RES_MEMORY] = memory;
  ns.dirty = true;
  return KE_OK;
}

int ke_node_set_cpuset_allocated(ke_ctx* ctx, int32_t node, int64_t cpus) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  ns.node.cpuset_allocated_cpus = cpus;
  ns.dirty = true;
  return KE_OK;
}

int ke_nodemetric_upsert(ke_ctx* ctx, int32_t node, const ke_node_metric* nm, int32_t n_pm, const ke_pod_metric* pm,
                         int32_t n_agg, const ke_aggregated_usage* agg) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  if (!nm || n_pm < 0 || n_agg < 0 || (n_pm && !pm) || (n_agg && !agg)) return fail(KE_ERR_INVALID, "nodemetric");
  NodeState& ns = ctx->c.nodes[node];
  ns.has_metric = true;
  ns.nm = *nm;
  ns.pm.assign(pm, pm + n_pm);
  ns.agg.assign(agg, agg + n_agg);
  ns.dirty = true;
  return KE_OK;
}

int ke_nodemetrics_load(ke_ctx* ctx, int32_t n, const ke_node_metric* nms, const int64_t* pm_offsets,
                        const ke_pod_metric* pod_metrics, const int64_t* agg_offsets, const ke_aggregated_usage* aggregated) {
  if (ctx) async_drain(ctx);
  if (!ctx || n < 0 || (n > 0 && (!nms || !pm_offsets || !agg_offsets))) return fail(KE_ERR_INVALID, "nodemetrics_load");
  if (ctx) flush_mirror(ctx->c);
  for (int32_t i = 0; i < n; i++) {
    const int64_t p0 = pm_offsets[i], p1 = pm_offsets[i + 1], a0 = agg_offsets[i], a1 = agg_offsets[i + 1];
    if (p1 < p0 || a1 < a0) return fail(KE_ERR_INVALID, "offsets must be non-decreasing");
    int rc = ke_nodemetric_upsert(ctx, i, &nms[i], (int32_t)(p1 - p0), pod_metrics ? pod_metrics + p0 : nullptr,
                                  (int32_t)(a1 - a0), aggregated ? aggregated + a0 : nullptr);
    if (rc) return rc;
  }
  return KE_OK;
}

int ke_nodemetric_delete(ke_ctx* ctx, int32_t node) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  ns.has_metric = false;
  ns.nm = ke_node_metric{};
  ns.pm.clear();
  ns.agg.clear();
  ns.dirty = true;
  return KE_OK;
}

int ke_pod_assign(ke_ctx* ctx, int32_t node, const ke_pod* pod, int64_t timestamp_ns) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  if (!pod) return fail(KE_ERR_INVALID, "null pod");
  host_assign(ctx->c.cfg, ctx->c.nodes[node], *pod, timestamp_ns);
  return KE_OK;
}

int ke_pods_assign(ke_ctx* ctx, int32_t n, const int32_t* nodes, const ke_pod* pods, const int64_t* timestamps_ns) {
  if (ctx) async_drain(ctx);
  if (!ctx || n < 0 || (n > 0 && (!nodes || !pods || !timestamps_ns))) return fail(KE_ERR_INVALID, "ke_pods_assign");
  if (ctx) flush_mirror(ctx->c);
  for (int32_t i = 0; i < n; i++) {
    int rc = check_node(ctx, nodes[i]);
    if (rc) return rc;
    host_assign(ctx->c.cfg, ctx->c.nodes[nodes[i]], pods[i], timestamps_ns[i]);
  }
  return KE_OK;
}

int ke_pod_unassign(ke_ctx* ctx, int32_t node, int64_t uid) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  NodeState& ns = ctx->c.nodes[node];
  for (size_t i = 0; i < ns.asg_uid.size(); i++) {
    if (ns.asg_uid[i] == uid) {
      ns.asg.erase(ns.asg.begin() + (long)i);
      ns.asg_uid.erase(ns.asg_uid.begin() + (long)i);
      ns.dirty = true;
      break;
    }
  }
  return KE_OK;
}

int ke_estimate_pod(ke_ctx* ctx, const ke_pod* pod, int64_t* est) {
  if (ctx) async_drain(ctx);
  if (!ctx || !pod || !est) return fail(KE_ERR_INVALID, "ke_estimate_pod arguments");
  uint8_t present[KE_NRES];
  estimate_pod(ctx->c.cfg.loadaware, *pod, est, present);
  for (int r = 0; r < KE_NRES; r++)
    if (!present[r]) est[r] = KE_ABSENT;
  return KE_OK;
}

int ke_eval(ke_ctx* ctx, int32_t n_pods, const ke_pod* pods, int64_t now_ns, uint8_t* status, uint8_t* reason,
            int16_t* la_score, int16_t* numa_score, int16_t* ds_score, int16_t* total, int32_t* best) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  if (ctx) flush_mirror(ctx->c);
  int rc = take_node_sets(ctx, n_pods, pods, false);
  if (rc) return rc;
  rc = check_pods(pods, n_pods, &ctx->c);
  if (rc) return rc;
  rc = check_numa_deviceshare(ctx, pods, n_pods);
  if (rc) return rc;
  rc = check_cpuset(ctx, pods, n_pods);
  if (rc) return rc;
  rc = require_device(ctx);
  if (rc) return rc;
  return device_eval(&ctx->c, n_pods, pods, now_ns, status, reason, la_score, numa_score, ds_score, total, best);
}

// The reductions of ke_eval's status / reason over every node, per pod (include/koord_eval.h).  ke_eval's admission in
// its order -- the staged set / table ids are consumed first, whatever follows -- then this call's own arguments.
int ke_diagnose(ke_ctx* ctx, int32_t n_pods, const ke_pod* pods, int64_t now_ns, ke_pod_diagnosis* out,
                int32_t words_per_pod, uint64_t* feasible, uint64_t* unschedulable, uint64_t* unresolvable) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  flush_mirror(ctx->c);
  int rc = take_node_sets(ctx, n_pods, pods, false, /*filter_only=*/true);  // (score offsets do not filter)
  if (rc) return rc;
  if (n_pods > 0 && !out) return fail(KE_ERR_INVALID, "diagnose: null out");
  if ((feasible || unschedulable || unresolvable) && words_per_pod < (ctx->c.n_nodes + 63) / 64)
    return fail(KE_ERR_INVALID, "diagnose: words_per_pod below ceil(ke_num_nodes / 64)");
  rc = check_pods(pods, n_pods, &ctx->c);
  if (rc) return rc;
  if (ctx->c.cfg.global_node_offset != 0 || (ctx->c.dev && device_sharded(&ctx->c)))
    return fail(KE_ERR_UNSUPPORTED, "diagnose: a node-sharded context");
  rc = check_numa_deviceshare(ctx, pods, n_pods);
  if (rc) return rc;
  rc = check_cpuset(ctx, pods, n_pods);
  if (rc) return rc;
  rc = require_device(ctx);
  if (rc) return rc;
  uint64_t* const bits[DIAG_BITMAPS] = {feasible, unschedulable, unresolvable};
  return device_diagnose(&ctx->c, n_pods, pods, now_ns, out, words_per_pod, bits);
}
const char* ke_reason_message(int32_t reason) { return diag_reason_message(reason); }
uint32_t ke_reason_plugin(int32_t reason) { return diag_reason_plugin(reason); }

// ---- resident pods, PDB budgets and ke_preempt (the table logic is ke_preempt.h's) -----------------------
int ke_resident_pods_load(ke_ctx* ctx, int32_t n_nodes, const int32_t* offsets, const ke_resident_pod* pods) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  const char* why = "";
  const int rc = resident_load(ctx->c.residents, n_nodes, offsets, pods, &why);
  return rc ? fail(rc, why) : KE_OK;
}
int ke_resident_pod_add(ke_ctx* ctx, int32_t node, const ke_resident_pod* pod) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  const char* why = "";
  const int rc = resident_add(ctx->c.residents, node, pod, &why);
  return rc ? fail(rc, why) : KE_OK;
}
int ke_resident_pod_remove(ke_ctx* ctx, int32_t node, int64_t uid) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  const char* why = "";
  const int rc = resident_remove(ctx->c.residents, node, uid, &why);
  return rc ? fail(rc, why) : KE_OK;
}
int ke_resident_pods_get(ke_ctx* ctx, int32_t node, int32_t cap, ke_resident_pod* out, int32_t* n) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  const char* why = "";
  const int rc = resident_get(ctx->c.residents, node, cap, out, n, &why);
  return rc ? fail(rc, why) : KE_OK;
}
int ke_pdbs_load(ke_ctx* ctx, int32_t n, const int32_t* disruptions_allowed) {
  if (ctx) async_drain(ctx);
  if (!ctx || n < 0 || n > 65535 || (n > 0 && !disruptions_allowed)) return fail(KE_ERR_INVALID, "ke_pdbs_load arguments");
  ctx->c.pdb_allowed.assign(disruptions_allowed, disruptions_allowed + n);
  ctx->c.pdb_dirty = true;
  return KE_OK;
}
int ke_abi_preempt_struct_sizes(int32_t* sizes, int32_t n) {
  const int32_t all[] = {(int32_t)sizeof(ke_resident_pod), (int32_t)sizeof(ke_preempt_args), (int32_t)sizeof(ke_preemption)};
  const int32_t m = (int32_t)(sizeof(all) / sizeof(all[0]));
  for (int32_t i = 0; i < n && i < m; i++) sizes[i] = all[i];
  return m;
}

// ke_diagnose's admission in its order (the staged ids are consumed first, whatever follows), then this call's own
// arguments and the refusals of everything but a plain preemptor; the per-preemptor uniforms are the host's.
int ke_preempt(ke_ctx* ctx, int32_t n_pods, const ke_pod* pods, const int32_t* priorities, int64_t now_ns,
               const ke_preempt_args* args, ke_preemption* out, int32_t victims_cap, int64_t* victim_uids,
               int32_t words_per_pod, uint64_t* candidates) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  Context& c = ctx->c;
  flush_mirror(c);
  int rc = take_node_sets(ctx, n_pods, pods, false, /*filter_only=*/true);  // (score offsets do not filter)
  if (rc) return rc;
  if (n_pods > 0 && (!out || !priorities || !victim_uids)) return fail(KE_ERR_INVALID, "preempt: null out, priorities or victim_uids");
  if (victims_cap < 1) return fail(KE_ERR_INVALID, "preempt: victims_cap below 1");
  if (candidates && words_per_pod < (c.n_nodes + 63) / 64)
    return fail(KE_ERR_INVALID, "preempt: words_per_pod below ceil(ke_num_nodes / 64)");
  const ke_preempt_args none{};
  const ke_preempt_args& a = args ? *args : none;
  if (a.default_quota < 0 || a.default_quota > (int32_t)c.quotas.size())
    return fail(KE_ERR_INVALID, "preempt: ke_preempt_args.default_quota outside the loaded ElasticQuota tree");
  rc = check_pods(pods, n_pods, &c);
  if (rc) return rc;
  for (int32_t p = 0; p < n_pods; p++)
    if (pods[p].quota < 0 || pods[p].quota > (int32_t)c.quotas.size())
      return fail(KE_ERR_INVALID, "ke_pod.quota outside the loaded ElasticQuota tree");
  auto no = [](const char* what) { return fail(KE_ERR_UNSUPPORTED, std::string("preempt: ") + what); };
  if (c.cfg.global_node_offset != 0 || (c.dev && device_sharded(&c))) return no("a node-sharded context");
  if (c.att.groups || c.att.domains || c.att.terms || c.att.dterms) return no("staged spread group / spread domain ids or term lists");
  if (c.numa_enabled || c.n_policy_nodes > 0) return no("a context with NUMA topology policy state");
  if (c.n_bind_nodes > 0) return no("a context with CPU bind policy nodes");
  for (int32_t p = 0; p < n_pods; p++) {
    if (pods[p].numa_topology_policy != KE_NUMA_POLICY_NONE) return no("a NUMA-policy pod");
    const DevPod dp = make_dev_pod(c.cfg, pods[p], pod_hints(c, pods[p]), &c.tmpl);
    if (dp.flags & (PF_DS | PF_DS_HINT | PF_DS_INVALID)) return no("a DeviceShare pod");
    if (dp.flags & (PF_CPUSET | PF_CPU_INVALID)) return no("a cpuset pod");
    for (int q = 0; q < NUM_XS; q++)
      if (((c.kargs_template.fit_scalar >> q) & 1) && dp.xreq[q] != 0)
        return no("a pod with a non-zero request for a scalar in ke_fit_args.scalars");
  }
  rc = check_cpuset(ctx, pods, n_pods);  // (stages the DevPod records; no pod of the call binds CPUs)
  if (rc) return rc;
  rc = require_device(ctx);
  if (rc) return rc;
  if (!device_preempt) return fail(KE_ERR_NO_DEVICE, "preempt: built without the device half");
  if (!c.quotas.empty() && (rc = device_quota_sync(&c))) return rc;  // the device holds the current used after a ke_schedule
  std::vector<PreemptPod> pre((size_t)n_pods);
  for (int32_t p = 0; p < n_pods; p++) {
    PreemptPod& u = pre[(size_t)p];
    u = PreemptPod{};
    u.priority = priorities[p];
    u.quota = (int16_t)pods[p].quota;
    u.blocked_quota = a.disable_default_quota_preemption ? a.default_quota : (int16_t)0;
    if (u.quota > 0) {
      const size_t qi = (size_t)u.quota - 1;
      const ke_quota& q = c.quotas[qi];
      for (int r = 0; r < KE_NRES; r++) {
        u.used[r] = q.used[r];
        u.lim[r] = c.qlimit[qi * KE_NRES + r];
        if (c.qlimit_has[qi * KE_NRES + r]) u.lim_has |= (uint8_t)(1u << r);
        if (q.has_max[r]) u.max_has |= (uint8_t)(1u << r);
        u.req[r] = q.has_max[r] ? pods[p].requests[r == 0 ? KE_RES_CPU : KE_RES_MEMORY] : 0;
      }
    }
  }
  return device_preempt(&c, n_pods, pods, pre.data(), now_ns, out, victims_cap, victim_uids, words_per_pod, candidates);
}

// check, plan (ke_segments.h), then per segment prepare -> device_schedule -> finish -> mirror -> append
static int schedule_sync(ke_ctx* ctx, int32_t n_pods, const ke_pod* pods, int64_t now_ns, int32_t* chosen, int32_t* score) {
  if (!ctx || (n_pods > 0 && !chosen)) return fail(KE_ERR_INVALID, "ke_schedule arguments");
  using clk = std::chrono::steady_clock;
  const auto tp = clk::now();
  Context& c = ctx->c;
  c.call_entry = tp;  // every pod of the call is dequeued now (ke_last_pod_latencies)
  int rc;  // every refusal is raised before any pod is scheduled
  if ((rc = check_pods(pods, n_pods, &c, true)) || (rc = check_numa_deviceshare(ctx, pods, n_pods)) ||
      (rc = check_cpuset(ctx, pods, n_pods)))
    return rc;
  for (int32_t p = 0; p < n_pods; p++)
    if (pods[p].quota < 0 || pods[p].quota > (int32_t)c.quotas.size())
      return fail(KE_ERR_INVALID, "ke_pod.quota outside the loaded ElasticQuota tree");
  if ((rc = check_matches(c, pods, n_pods)) || (rc = require_device(ctx))) return rc;
  c.host_ms[0] = std::chrono::duration<double, std::milli>(clk::now() - tp).count();
  std::vector<uint8_t> cls((size_t)n_pods, 0);  // PodClass bits
  const bool barriers = !c.quotas.empty() && c.qargs.enable_runtime_quota;
  for (int32_t p = 0; p < n_pods; p++) {
    const bool ignored = pods[p].reservation_matched == KE_RSV_IGNORED;
    const bool matched = pods[p].reservation_matched == KE_RSV_AFFINITY ||
                         (!c.match_off.empty() && c.match_off[(size_t)p + 1] > c.match_off[(size_t)p]);
    if (barriers && pods[p].quota > 0 && c.quotas[(size_t)pods[p].quota - 1].limit_is_max) cls[(size_t)p] |= PC_BARRIER;
    if (matched || (ignored && resv_ignore_needs_views(c, pods[p], c.staged[(size_t)p].flags))) cls[(size_t)p] |= PC_ALONE;
    if (ignored) cls[(size_t)p] |= PC_IGNORED;
  }
  const std::vector<Segment> segs = plan_segments(n_pods, cls.data());
  CallRecords all;  // the segments' records joined; resv: what each matched pod was assumed into
  CallTimes times;
  all.resv.assign((size_t)n_pods, 0);
  c.last_rsv_fused = c.last_rsv_fused_gated = 0;
  for (size_t k = 0; k < segs.size(); k++) {
    SegmentRun run{c, pods, n_pods, now_ns, chosen, score, all.resv.data(), cls.data(), segs[k]};
    if ((rc = run.prepare()) || (rc = run.schedule()) || (rc = run.finish())) return rc;
    if (n_pods == 0) break;  // (the empty call still refreshes the rows)
    run.mirror();
    all.append(c.last, (size_t)run.len);
    times.add(c.last_total_ms, c.last_batch_ms, c.last_pod_lat);
    if ((rc = run.refresh_quota())) return rc;
    k += run.fuse;  // (the next segment was the fused pod)
  }
  all.set_pods(n_pods, chosen, pods, !c.quotas.empty(), c.resv_gen);
  c.last = std::move(all);
  c.last_total_ms = times.total_ms;
  c.last_batch_ms.swap(times.batch_ms);
  c.last_pod_lat.swap(times.pod_lat);
  return KE_OK;
}

int ke_schedule(ke_ctx* ctx, int32_t n_pods, const ke_pod* pods, int64_t now_ns, int32_t* chosen, int32_t* score) {
  if (!ctx) return fail(KE_ERR_INVALID, "ke_schedule arguments");
  async_drain(ctx);
  const StagedMatches consumed{ctx->c};
  int rc = take_node_sets(ctx, n_pods, pods, true);
  if (!rc) rc = take_gangs(ctx, n_pods, pods);
  else ctx->c.pod_gangs.take();
  if (rc) return rc;
  return schedule_sync(ctx, n_pods, pods, now_ns, chosen, score);
}

int ke_schedule_submit(ke_ctx* ctx, int32_t n_pods, const ke_pod* pods, int64_t now_ns, int64_t* ticket) {
  if (!ctx || n_pods < 0 || (n_pods > 0 && !pods) || !ticket) return fail(KE_ERR_INVALID, "ke_schedule_submit arguments");
  using clk = std::chrono::steady_clock;
  Context& c = ctx->c;
  const StagedMatches consumed{c};
  {
    int rc = take_node_sets(ctx, n_pods, pods, true);
    if (!rc) rc = take_gangs(ctx, n_pods, pods);
    else c.pod_gangs.take();
    if (rc) return rc;
  }
  int in_flight = 0;
  for (const AsyncCall& a : ctx->async) in_flight += a.fin != nullptr;
  // at most one call in flight behind which this one is enqueued (two sets of call buffers)
  for (AsyncCall& a : ctx->async)
    if (in_flight >= 2 && a.fin) async_finish(ctx, a), in_flight--;
  // a plain queue: no reservation-matched, NUMA-policy or quota pod, no staged reservation lists
  bool plain = c.dev && n_pods > 0 && c.match_off.empty() && c.quotas.empty() && !c.numa_enabled;
  for (int32_t p = 0; p < n_pods && plain; p++)
    plain = pods[p].reservation_matched == KE_RSV_NONE && pods[p].numa_topology_policy == KE_NUMA_POLICY_NONE &&
            pods[p].quota == 0;
  if (plain) {
    const auto tp = clk::now();
    int rc = check_pods(pods, n_pods, &c);
    if (rc) return rc;
    rc = check_cpuset(ctx, pods, n_pods);  // (stages the pods' records)
    if (rc) return rc;
    plain = device_async_ok(&c, n_pods);
    if (plain && in_flight > 0 && device_refresh_pending(&c, now_ns)) {
      async_drain(ctx);  // rows to derive from the host state: it must carry the Reserves of the calls in flight
      in_flight = 0;
    }
    if (plain) {
      c.call_entry = tp;
      c.host_ms[0] = std::chrono::duration<double, std::milli>(clk::now() - tp).count();
      if (in_flight > 0) device_swap_call_buffers(&c);  // (the call in flight keeps its own)
      AsyncCall a;
      a.ticket = ctx->next_ticket++;
      a.n = n_pods;
      a.pods = pods;
      a.now = now_ns;
      a.device = true;
      c.call_behind = in_flight > 0;
      rc = device_schedule_enqueue(&c, n_pods, pods, now_ns, true, &a.fin);
      if (rc) {
        // the call in flight keeps the buffers its completion captured: swap back, and let no partly enqueued
        // launch of this call outlive the error
        if (in_flight > 0) device_swap_call_buffers(&c);
        device_quiesce(&c);
        return rc;
      }
      *ticket = a.ticket;
      ctx->async.push_back(std::move(a));
      return KE_OK;
    }
  }
  // anything else runs now, after every call in flight
  async_drain(ctx);
  AsyncCall a;
  a.ticket = ctx->next_ticket++;
  a.n = n_pods;
  a.pods = pods;
  a.now = now_ns;
  a.chosen.assign((size_t)n_pods, -1);
  a.score.assign((size_t)n_pods, 0);
  const int rc = schedule_sync(ctx, n_pods, pods, now_ns, a.chosen.data(), a.score.data());
  if (rc) return rc;
  a.rec = c.last;
  *ticket = a.ticket;
  ctx->async.push_back(std::move(a));
  return KE_OK;
}

int ke_schedule_wait(ke_ctx* ctx, int64_t ticket, int32_t* chosen, int32_t* score) {
  if (!ctx) return fail(KE_ERR_INVALID, "ke_schedule_wait arguments");
  size_t i = 0;
  while (i < ctx->async.size() && ctx->async[i].ticket != ticket) i++;
  if (i == ctx->async.size()) return fail(KE_ERR_NOT_FOUND, "ke_schedule_wait: no such submitted call");
  if (ctx->async[i].n > 0 && !chosen) return fail(KE_ERR_INVALID, "ke_schedule_wait arguments");
  for (size_t j = 0; j <= i; j++) async_finish(ctx, ctx->async[j]);  // (in submission order)
  AsyncCall a = std::move(ctx->async[i]);
  ctx->async.erase(ctx->async.begin() + (long)i);
  if (a.rc) return fail(a.rc, a.msg);
  std::copy(a.chosen.begin(), a.chosen.end(), chosen);
  if (score) std::copy(a.score.begin(), a.score.end(), score);
  // release records of this call (ke_last_allocations / ke_unreserve): the last collected call, device-enqueued
  // or run at once alike
  ctx->c.last.restore(std::move(a.rec), ctx->c.resv_gen);
  return KE_OK;
}

int ke_last_allocations(ke_ctx* ctx, int32_t n, ke_pod_allocation* out) {
  if (!ctx || n < 0 || (n > 0 && !out)) return fail(KE_ERR_INVALID, "ke_last_allocations arguments");
  for (int32_t p = 0; p < n; p++) out[p] = ctx->c.last.allocation(p, ctx->c.resv_gen, ctx->c.resv);
  return KE_OK;
}

int ke_pod_release(ke_ctx* ctx, const ke_pod* pod, const ke_pod_allocation* alloc, int32_t mode) {
  if (ctx) async_drain(ctx);
  if (!ctx || !pod || !alloc) return fail(KE_ERR_INVALID, "ke_pod_release arguments");
  if (mode != KE_RELEASE_UNRESERVE && mode != KE_RELEASE_DELETE) return fail(KE_ERR_INVALID, "ke_pod_release mode");
  int rc = validate_pod(*pod);
  if (rc) return rc;
  Context& c = ctx->c;
  rc = validate_pod_hints(c, *pod);
  if (rc) return rc;
  flush_mirror(c);  // the pod's own deferred Reserve mirror first
  if (pod->quota < 0 || pod->quota > (int32_t)c.quotas.size())
    return fail(KE_ERR_INVALID, "ke_pod.quota outside the loaded ElasticQuota tree");
  const int32_t node = alloc->node < 0 ? -1 : alloc->node - c.cfg.global_node_offset;
  if (node >= c.cfg.node_capacity) return fail(KE_ERR_NOT_FOUND, "ke_pod_release: node index out of range");
  // the reservation the pod was assumed into: by uid (the set may have been reloaded since), else by an index of
  // the current set
  int32_t ridx = -1;
  if (alloc->reservation > 0 && alloc->reservation_uid != 0) {
    for (size_t i = 0; i < c.resv.size() && ridx < 0; i++)
      if (c.resv[i].uid == alloc->reservation_uid) ridx = (int32_t)i;
  } else if (alloc->reservation > 0) {
    if (alloc->reservation > (int32_t)c.resv.size()) return fail(KE_ERR_NOT_FOUND, "ke_pod_release: reservation index");
    if (alloc->reservation_generation != c.resv_gen)
      return fail(KE_ERR_INVALID, "ke_pod_release: a reservation index of an earlier reservation set (no uid)");
    ridx = alloc->reservation - 1;
  } else if (alloc->reservation < 0) {
    return fail(KE_ERR_NOT_FOUND, "ke_pod_release: reservation index");
  }
  if (node >= 0 && c.nodes[(size_t)node].known)  // (also a deleted node: its caches keep the pod until released)
    host_release_node(c.cfg, c.ext_enabled, c.nodes[(size_t)node], *pod, *alloc, pod_hints(c, *pod));
  if (node >= 0 && ridx >= 0) resv_forget(c, ridx, *pod, alloc);
  const bool assigned = alloc->node >= 0 && alloc->quota_assigned;
  if (pod->quota > 0 && (assigned || mode == KE_RELEASE_DELETE)) {
    if (c.dev) {
      rc = device_quota_sync(&c);  // the device holds the current used after a ke_schedule
      if (rc) return rc;
    }
    rc = host_quota_release(c, *pod, assigned, mode == KE_RELEASE_DELETE);
    if (rc) return rc;
  }
  return KE_OK;
}

int ke_unreserve(ke_ctx* ctx, const ke_pod* pod, int32_t queue_pos) {
  if (ctx) async_drain(ctx);
  if (!ctx || !pod) return fail(KE_ERR_INVALID, "ke_unreserve arguments");
  Context& c = ctx->c;
  if (queue_pos < 0 || queue_pos >= (int32_t)c.last.chosen.size())
    return fail(KE_ERR_NOT_FOUND, "ke_unreserve: no such position in the last ke_schedule");
  if (c.last.uid[(size_t)queue_pos] != pod->uid) return fail(KE_ERR_INVALID, "ke_unreserve: pod uid differs from the queue's");
  if (c.last.chosen[(size_t)queue_pos] < 0) return KE_OK;  // not placed, or already unreserved
  const ke_pod_allocation a = c.last.allocation(queue_pos, c.resv_gen, c.resv);
  const int rc = ke_pod_release(ctx, pod, &a, KE_RELEASE_UNRESERVE);
  if (rc) return rc;
  c.last.chosen[(size_t)queue_pos] = -1;
  return KE_OK;
}

int ke_last_pod_latencies(ke_ctx* ctx, int32_t n, double* ms) {
  if (!ctx || n < 0 || (n > 0 && !ms)) return fail(KE_ERR_INVALID, "ke_last_pod_latencies arguments");
  const auto& v = ctx->c.last_pod_lat;
  for (int32_t i = 0; i < n; i++) ms[i] = i < (int32_t)v.size() ? v[(size_t)i] : 0.0;
  return KE_OK;
}

int ke_last_host_stats(ke_ctx* ctx, double* ms8) {
  if (!ctx || !ms8) return fail(KE_ERR_INVALID, "ke_last_host_stats arguments");
  for (int i = 0; i < 8; i++) ms8[i] = ctx->c.host_ms[i];
  return KE_OK;
}

int ke_last_schedule_stats(ke_ctx* ctx, double* total_ms, int32_t* n_batches, double* batch_ms, int32_t batch_ms_cap) {
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  if (total_ms) *total_ms = ctx->c.last_total_ms;
  if (n_batches) *n_batches = (int32_t)ctx->c.last_batch_ms.size();
  if (batch_ms) {
    const int32_t n = std::min<int32_t>(batch_ms_cap, (int32_t)ctx->c.last_batch_ms.size());
    for (int32_t i = 0; i < n; i++) batch_ms[i] = ctx->c.last_batch_ms[i];
  }
  return KE_OK;
}

int ke_set_profiling(ke_ctx* ctx, int32_t sample_every) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  int rc = require_device(ctx);
  if (rc) return rc;
  return device_set_profiling(&ctx->c, sample_every);
}

int ke_last_kernel_stats(ke_ctx* ctx, double* eval_ms, double* select_ms, double* resolve_ms, int32_t* samples) {
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  if (eval_ms) *eval_ms = ctx->c.kstat_eval_ms;
  if (select_ms) *select_ms = ctx->c.kstat_select_ms;
  if (resolve_ms) *resolve_ms = ctx->c.kstat_resolve_ms;
  if (samples) *samples = ctx->c.kstat_samples;
  return KE_OK;
}

int ke_last_kernel_stats_ex(ke_ctx* ctx, double* ms4 /* [8] */, int32_t* samples, int32_t* pipelined_batches) {
  if (!ctx || !ms4) return fail(KE_ERR_INVALID, "ke_last_kernel_stats_ex arguments");
  ms4[0] = ctx->c.kstat_eval_ms;
  ms4[1] = ctx->c.kstat_select_ms;
  ms4[2] = ctx->c.kstat_fixup_ms;
  ms4[3] = ctx->c.kstat_resolve_ms;
  if (samples) *samples = ctx->c.kstat_samples;
  if (pipelined_batches) *pipelined_batches = ctx->c.last_pipelined;
  ms4[4] = ctx->c.last_enqueue_ms;
  ms4[5] = ctx->c.kstat_handoff_ms;
  ms4[6] = ctx->c.kstat_rows_fetched;
  ms4[7] = ctx->c.kstat_rows_changed;
  return KE_OK;
}

int ke_debug_replay_phases(ke_ctx* ctx, double* cyc8) {
  if (ctx) async_drain(ctx);
  if (!ctx || !cyc8) return fail(KE_ERR_INVALID, "ke_debug_replay_phases arguments");
  int rc = require_device(ctx);
  if (rc) return rc;
  return device_replay_phases(&ctx->c, 0, cyc8);
}

int ke_debug_kernel_phases(ke_ctx* ctx, int32_t kernel, double* cyc8) {
  if (ctx) async_drain(ctx);
  if (!ctx || !cyc8 || kernel < 0 || kernel > 3) return fail(KE_ERR_INVALID, "ke_debug_kernel_phases arguments");
  int rc = require_device(ctx);
  if (rc) return rc;
  return device_replay_phases(&ctx->c, kernel, cyc8);
}

int ke_debug_spec_failed(ke_ctx* ctx, double* per_batch) {
  if (!ctx || !per_batch) return fail(KE_ERR_INVALID, "ke_debug_spec_failed arguments");
  *per_batch = ctx->c.kstat_spec_failed;
  return KE_OK;
}

int ke_debug_call_boundary(ke_ctx* ctx, int64_t* out4) {
  if (!ctx || !out4) return fail(KE_ERR_INVALID, "ke_debug_call_boundary arguments");
  for (int i = 0; i < 4; i++) out4[i] = ctx->c.call_boundary[i];
  return KE_OK;
}

int ke_debug_check_records(ke_ctx* ctx, int64_t now_ns, int64_t* mismatched_nodes) {
  if (ctx) async_drain(ctx);
  if (!ctx || !mismatched_nodes) return fail(KE_ERR_INVALID, "ke_debug_check_records arguments");
  flush_mirror(ctx->c);
  int rc = require_device(ctx);
  if (rc) return rc;
  return device_check_records(&ctx->c, now_ns, mismatched_nodes);
}

int ke_debug_spread_groups_check(ke_ctx* ctx, int64_t* mismatched) {
  if (ctx) async_drain(ctx);
  if (!ctx || !mismatched) return fail(KE_ERR_INVALID, "ke_debug_spread_groups_check arguments");
  *mismatched = 0;
  if (!ctx->c.dev || !device_spread_groups_check) return KE_OK;  // (no device copy yet)
  return device_spread_groups_check(&ctx->c, mismatched);
}

int ke_debug_spread_domains_check(ke_ctx* ctx, int64_t* mismatched) {
  if (ctx) async_drain(ctx);
  if (!ctx || !mismatched) return fail(KE_ERR_INVALID, "ke_debug_spread_domains_check arguments");
  *mismatched = 0;
  if (!ctx->c.dev || !device_spread_domains_check) return KE_OK;  // (no device copy yet)
  return device_spread_domains_check(&ctx->c, mismatched);
}

int ke_debug_devices_check(ke_ctx* ctx, int64_t* mismatched_nodes) {
  if (ctx) async_drain(ctx);
  if (!ctx || !mismatched_nodes) return fail(KE_ERR_INVALID, "ke_debug_devices_check arguments");
  *mismatched_nodes = 0;
  flush_mirror(ctx->c);
  if (!ctx->c.dev || !device_devices_check) return KE_OK;  // (no device copy yet)
  return device_devices_check(&ctx->c, mismatched_nodes);
}

int ke_set_pipeline(ke_ctx* ctx, int32_t on) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  int rc = require_device(ctx);
  if (rc) return rc;
  return device_set_pipeline(&ctx->c, on);
}

int ke_last_resolve_split(ke_ctx* ctx, double* prologue_ms, double* replay_ms) {
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  if (prologue_ms) *prologue_ms = ctx->c.kstat_resolve_prologue_ms;
  if (replay_ms) *replay_ms = ctx->c.kstat_resolve_loop_ms;
  return KE_OK;
}

int ke_debug_numa_deferred(ke_ctx* ctx, int64_t* n) {
  if (!ctx || !n) return fail(KE_ERR_INVALID, "ke_debug_numa_deferred arguments");
  *n = ctx->c.kstat_numa_deferred;
  return KE_OK;
}

int ke_debug_resolve_phases(ke_ctx* ctx, double* phases6) {
  if (!ctx || !phases6) return fail(KE_ERR_INVALID, "ke_debug_resolve_phases arguments");
  for (int i = 0; i < 6; i++) phases6[i] = ctx->c.kstat_resolve_phase_ms[i];
  return KE_OK;
}

int ke_debug_resolve_subphases(ke_ctx* ctx, double* sub5) {
  if (!ctx || !sub5) return fail(KE_ERR_INVALID, "ke_debug_resolve_subphases arguments");
  for (int i = 0; i < 5; i++) sub5[i] = ctx->c.kstat_resolve_sub_ms[i];
  return KE_OK;
}

int ke_debug_resolve_wave1(ke_ctx* ctx, double* w4) {
  if (!ctx || !w4) return fail(KE_ERR_INVALID, "ke_debug_resolve_wave1 arguments");
  for (int i = 0; i < 4; i++) w4[i] = ctx->c.kstat_resolve_wave1_ms[i];
  return KE_OK;
}

int ke_bench_eval_kernel(ke_ctx* ctx, int32_t n_pods, const ke_pod* pods, int64_t now_ns, int32_t iters,
                         double* avg_ms) {
  if (ctx) async_drain(ctx);
  if (!ctx || !avg_ms) return fail(KE_ERR_INVALID, "ke_bench_eval_kernel arguments");
  if (ctx) flush_mirror(ctx->c);
  int rc = check_pods(pods, n_pods);
  if (rc) return rc;
  rc = require_device(ctx);
  if (rc) return rc;
  return device_bench_eval(&ctx->c, n_pods, pods, now_ns, iters, avg_ms);
}

int ke_comm_unique_id(uint8_t* id, int32_t id_bytes) {
  if (!id || id_bytes < KE_COMM_ID_BYTES) return fail(KE_ERR_INVALID, "ke_comm_unique_id: need a 128-byte buffer");
  if (!device_available()) return fail(KE_ERR_NO_DEVICE, "ke_comm_unique_id: no HIP device");
  return device_comm_unique_id(id);
}

int ke_shard_init(ke_ctx* ctx, int32_t rank, int32_t world, const uint8_t* id) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  int rc = require_device(ctx);
  if (rc) return rc;
  return device_shard_init(&ctx->c, rank, world, id);
}

int ke_shard_init_host(ke_ctx* ctx, int32_t rank, int32_t world, ke_host_collective fn, void* user) {
  if (ctx) async_drain(ctx);
  if (!ctx) return fail(KE_ERR_INVALID, "null context");
  int rc = require_device(ctx);
  if (rc) return rc;
  return device_shard_init_host(&ctx->c, rank, world, fn, user);
}

int ke_shard_range(ke_ctx* ctx, int32_t* lo, int32_t* hi) {
  if (ctx) async_drain(ctx);
  if (!ctx || !lo || !hi) return fail(KE_ERR_INVALID, "ke_shard_range arguments");
  int rc = require_device(ctx);
  if (rc) return rc;
  int l = 0, h = 0;
  rc = device_shard_range(&ctx->c, &l, &h);
  *lo = l;
  *hi = h;
  return rc;
}

int ke_debug_node_state(ke_ctx* ctx, int32_t node, ke_node* out, int32_t cpu_cap, ke_cpu* cpus, int32_t* n_cpus,
                        int32_t zone_cap, ke_numa_zone* zones, int32_t* n_zones, int32_t dev_cap, ke_device* devs,
                        int32_t* n_devs) {
  if (ctx) async_drain(ctx);
  int rc = check_node(ctx, node);
  if (ctx) flush_mirror(ctx->c);
  if (rc) return rc;
  const NodeState& ns = ctx->c.nodes[(size_t)node];
  if (out) *out = ns.node;
  if (n_cpus) *n_cpus = (int32_t)ns.cpus.size();
  for (int32_t i = 0; cpus && i < cpu_cap && i < (int32_t)ns.cpus.size(); i++) cpus[i] = ns.cpus[(size_t)i];
  if (n_zones) *n_zones = (int32_t)ns.zones.size();
  for (int32_t i = 0; zones && i < zone_cap && i < (int32_t)ns.zones.size(); i++) zones[i] = ns.zones[(size_t)i];
  if (n_devs) *n_devs = (int32_t)ns.devs.size();
  for (int32_t i = 0; devs && i < dev_cap && i < (int32_t)ns.devs.size(); i++) devs[i] = ns.devs[(size_t)i];
  return KE_OK;
}

int64_t ke_debug_usage_bound(int64_t total, int64_t thr) { return total > 0 ? max_used_within(total, thr) : 0; }

int ke_debug_rows(ke_ctx* ctx, int32_t n, int64_t now_ns, void* device_rows, void* host_rows) {
  if (ctx) async_drain(ctx);
  if (!ctx || n < 0 || n > ctx->c.n_nodes) return fail(KE_ERR_INVALID, "ke_debug_rows arguments");
  if (ctx) flush_mirror(ctx->c);
  if (device_rows) {
    int rc = require_device(ctx);
    if (rc) return rc;
    rc = device_debug_rows(&ctx->c, n, (Row*)device_rows);
    if (rc) return rc;
  }
  if (host_rows) {
    Row* out = (Row*)host_rows;
    for (int32_t i = 0; i < n; i++) {
      int64_t vu;
      derive_row(ctx->c.cfg, ctx->c.nodes[i], now_ns, &out[i], &vu);
    }
  }
  return KE_OK;
}

}  // extern "C"
