// The host plan of a ke_schedule call, free of HIP: the select's geometry (shared with the kernels), the batch
// segmentation and the pipelined runs, the per-batch select plan, the three staging layouts and the arithmetic of
// the call's statistics.  ke_kernels.hip includes it; tests/plan/plan_check.cpp compiles it alone with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "ke_gang.h"
#include "ke_types.h"

#ifndef KE_HD
#define KE_HD __host__ __device__
#endif

namespace ke {

// ---- geometry --------------------------------------------------------------------------------------------------------
constexpr int PST = 16;  // replay stamps / counters per batch (ke_debug_resolve_phases)
constexpr int SELECT_BLOCK = 1024;
constexpr int SELECT_WAVES = SELECT_BLOCK / 64;
constexpr int KMAX = MAX_BATCH;
constexpr int KSTALE = 2 * KMAX;   // stale-snapshot list length of the pipelined schedule
constexpr int KSTALE2 = 3 * KMAX;  // select-ahead list length (k_fixlist: up to KMAX of them are batch b-2's nodes)
constexpr int SEL_RC = 8;  // register-resident select: up to SEL_RC * 512 nodes per wave (65,536 per pod)
constexpr int MAX_WORLD = 8;
constexpr int EVAL_PPB = 8;  // pods per block (eval_grid's pod groups)
constexpr int gath_words(int L) { return MAX_BATCH * L + MAX_BATCH; }

// A plain batch of more than 2 pods is evaluated from the 208-B replay records (k_eval_plain: no int64 ->
// double work per pair, the record read once per 8 pods); 1-2 pods stream the 148-B SoA rows
// (k_eval_batch), the smaller read when the pass is bandwidth-bound.
KE_HD constexpr bool use_record_eval(int pods) { return pods > 2; }

// per-wave node segment of k_select over [lo, hi): a multiple of 512 (one 16-B load per lane per step)
KE_HD inline int select_seg(int lo, int hi) { return ((hi - lo + SELECT_WAVES - 1) / SELECT_WAVES + 511) & ~511; }
// node part of one of `parts` workgroups of a split k_select (512-aligned, like the shard ranges)
KE_HD inline int select_part(int lo, int hi, int parts) { return ((hi - lo + parts - 1) / parts + 511) & ~511; }
// register-resident when a wave's segment fits SEL_RC steps, else streamed
inline bool select_resident(int lo, int hi) { return select_seg(lo, hi) <= SEL_RC * 512; }

// KOORDEVAL_SELECT_PARTS = P, an A/B knob: at most P parts of >= 4096 nodes (unset: 8 parts of >= 24576)
struct SelectKnob {
  int cap = 8;
  int64_t per = 24576;
};
inline SelectKnob select_knob(const char* env) {
  return env ? SelectKnob{std::max(1, std::min(8, std::atoi(env))), 4096} : SelectKnob{};
}
// workgroups per pod of a plain batch's split k_select over n nodes: >= 256 workgroups in all, parts of
// >= 4096 nodes, at most MAX_WORLD (k_merge's fan-in)
// (parts of >= 24576 nodes: at C3's 50k nodes two parts per pod measured 93.5 G against 92.1 G with four and 91.1 G
// with one -- profiles/r06/ab_select_parts.txt; the split's merge tail costs more than the per-part pass saves.)
inline int select_parts(int64_t n, int bp, int L, SelectKnob kb) {
  static_assert(MAX_WORLD == 8, "select_parts caps the parts at 8");
  return std::max(1, std::min({kb.cap, (255 + bp) / bp, (int)(n / kb.per), 1024 / L}));  // (the merge: parts x L <= 1024)
}

// Contiguous node range of shard `rank`: 512-aligned chunks (k_select's 16-B loads stay aligned).
inline void shard_range(int n_nodes, int rank, int world, int* lo, int* hi) {
  const int chunk = ((n_nodes + world - 1) / world + 511) & ~511;
  *lo = std::min(rank * chunk, n_nodes);
  *hi = std::min(*lo + chunk, n_nodes);
}

// ---- batches and runs ------------------------------------------------------------------------------------------------
struct Batch {
  int pods;
  bool ds, cpu;  // DeviceShare-capable batch (its pods' NormalizeScore) / singleton of a pod that may bind CPUs
  bool cut;      // a DeviceShare batch with DeviceShare pods: the replay may stop early
  bool hint;     // singleton of a pod with device hints: its eval kernel carries the hint path (H)
  // a pod of the batch names a spread group: the batch runs serially on the one-wave sequential
  // replay, whose Reserves increment the group's per-node counts; never part of a pipelined run
  bool grouped = false;
};

// Batches: runs of up to B pods (exact speculative batching).  A pod that may bind CPUs is alone in
// its batch: its Reserve runs the CPU accumulator (k_cpuset_reserve) and may fail, and later pods read the CPU table
// it patches.  Hinted pods and a fused matched pod (the last one) are singletons too.  DeviceShare pods share batches
// (exact: the replay checks each pod's normalisation max and stops the batch where it may have moved)
// when `ds_batch` -- unsharded nodes without NUMA policies -- else each is a singleton: its NormalizeScore needs
// the max over all feasible nodes of the current state.
// `group_ids` (the call's spread group id per pod, nullptr: none): the segmentation is the same with or without them; a
// batch holding a pod with a non-zero id is marked `grouped`.
// `domain_ids` (the call's spread domain group id per pod; nullptr: none): a batch holds at most one pod
// of any spread domain group -- it ends before a pod whose non-zero id already occurs in it, so the group's domain
// counts during the batch are those of the batch's snapshot -- and a batch holding such a pod is `grouped` too.  With
// every id zero the plan is the one without them.
// `dterms` (the call's spread domain term record per pod; nullptr: none): a batch ends before a pod one
// of whose term groups is a member group of an earlier pod of that batch, so every group a pod reads keeps its snapshot
// counts for the whole batch (reads after reads, writes after writes and writes after reads share a batch).  The
// `grouped` mark of such a batch comes with `group_ids`.  With every record empty the plan is the one without them.
// `gangs` (the call's gang word per pod, ke_gang.h; nullptr: none): a run lies in one batch -- a batch
// ends before a run that would not fit in it whole (*gang_cuts counts these) -- a batch holding a member holds no
// DeviceShare pod (a DSB_CUT in mid-run would lose the run's state), and it is `grouped`.  Batches without a member are
// planned as without the words, and with every word zero the plan is the one without them.
// `gang_devices` (ke_set_gang_devices; DESIGN.md §4w, "DeviceShare members"): a member may be a DeviceShare pod and share
// its batch with DeviceShare pods -- the replay keeps the run's state across a DSB_CUT -- so that rule is dropped; the
// batch stays `grouped`, and `cut` as any DeviceShare batch of more than one pod.
inline std::vector<Batch> plan_batches(const DevPod* pods, int n_pods, int B, bool ds_batch, bool fused,
                                       const int32_t* group_ids = nullptr, const int32_t* domain_ids = nullptr,
                                       const PodTerms* dterms = nullptr, const int32_t* gangs = nullptr,
                                       int* gang_cuts = nullptr, bool gang_devices = false) {
  std::vector<Batch> batches;
  if (gang_cuts) *gang_cuts = 0;
  bool has_gang = false, has_ds = false;  // of the batch being filled
  // pod p0 + bp may not join the bp pods from p0 on: a run that does not fit whole, or a member beside a DeviceShare pod
  auto gang_stop = [&](int p0, int bp) {
    if (!gangs || bp == 0) return false;
    const int32_t w = gangs[p0 + bp];
    if ((w & GW_FIRST) && bp + gang_run_len(gangs, n_pods, p0 + bp) > B) {
      if (gang_cuts) (*gang_cuts)++;
      return true;
    }
    const bool ds = (pods[p0 + bp].flags & PF_DS) != 0;
    return !gang_devices && (((w & GW_MEMBER) && has_ds) || (ds && has_gang));
  };
  // pod p0 + bp reads a spread domain group that one of the bp pods from p0 on is a member of
  auto reads_written = [&](int p0, int bp) {  // (called with domain lists only)
    const PodTerms& r = dterms[p0 + bp];
    for (int t = 0; t < POD_TERMS && st_kind(r, t); t++)
      for (int q = 0; q < bp; q++)
        for (int m = 0; m < POD_MEMBERS; m++)
          if (st_member(dterms[p0 + q], m) == st_group(r, t)) return true;
    return false;
  };
  // pod p0 + bp names a spread domain group that one of the bp pods from p0 on names already
  auto repeats = [&](int p0, int bp) {
    const int32_t id = domain_ids ? domain_ids[p0 + bp] : 0;
    if (id == 0) return false;
    for (int q = 0; q < bp; q++)
      if (domain_ids[p0 + q] == id) return true;
    return false;
  };
  auto alone = [&](uint32_t f) { return (f & PF_CPUSET) || ((f & PF_DS) && !ds_batch) || (f & PF_DS_HINT); };
  for (int p = 0; p < n_pods;) {
    const uint32_t f = pods[p].flags;
    if (alone(f) || (fused && p == n_pods - 1)) {
      batches.push_back({1, (f & PF_DS) != 0, (f & PF_CPUSET) != 0, false, (f & PF_DS_HINT) != 0});
      p++;
      continue;
    }
    int bp = 0;
    has_ds = has_gang = false;
    while (p + bp < n_pods && bp < B && !(fused && p + bp == n_pods - 1) && !alone(pods[p + bp].flags) &&
           !repeats(p, bp) && (!dterms || !reads_written(p, bp)) && !gang_stop(p, bp)) {
      has_ds = has_ds || (pods[p + bp].flags & PF_DS);
      has_gang = has_gang || (gangs && (gangs[p + bp] & GW_MEMBER));
      bp++;
    }
    batches.push_back({bp, has_ds, false, has_ds && bp > 1, false});
    p += bp;
  }
  if (group_ids)
    for (size_t b = 0, p = 0; b < batches.size(); p += (size_t)batches[b].pods, b++)
      for (int q = 0; q < batches[b].pods; q++) batches[b].grouped = batches[b].grouped || group_ids[p + (size_t)q] != 0;
  if (domain_ids)
    for (size_t b = 0, p = 0; b < batches.size(); p += (size_t)batches[b].pods, b++)
      for (int q = 0; q < batches[b].pods; q++) batches[b].grouped = batches[b].grouped || domain_ids[p + (size_t)q] != 0;
  if (gangs)
    for (size_t b = 0, p = 0; b < batches.size(); p += (size_t)batches[b].pods, b++)
      for (int q = 0; q < batches[b].pods; q++) batches[b].grouped = batches[b].grouped || (gangs[p + (size_t)q] & GW_MEMBER);
  return batches;
}

// first pod of every batch and the end (the kernels' batch base pointer is d_bases + b)
inline std::vector<int32_t> plan_bases(const std::vector<Batch>& batches) {
  std::vector<int32_t> bases(batches.size() + 1);
  int32_t p = 0;
  for (size_t b = 0; b < batches.size(); b++) bases[b] = p, p += batches[b].pods;
  bases[batches.size()] = p;
  return bases;
}

// pipelined runs: maximal stretches of plain batches (no DeviceShare / cpuset pod, not the fused
// one, not a grouped batch) in a context without NUMA policies; run_end[b] > 0 marks the first batch of a run and holds its end
// (a lone plain batch between singletons gains nothing from the second stream: it runs serially)
inline std::vector<int> plan_runs(const std::vector<Batch>& batches, bool pipeline, int n_nodes, bool numa, bool fused) {
  const int nb = (int)batches.size();
  auto eligible = [&](int b) {
    return pipeline && n_nodes > 0 && !numa && !batches[b].ds && !batches[b].cpu && !batches[b].grouped &&
           !(fused && b == nb - 1);
  };
  std::vector<int> run_end((size_t)nb, 0);
  for (int b = 0; b < nb;) {
    int e = b;
    while (e < nb && eligible(e)) e++;
    if (e - b >= 2) run_end[b] = e;
    b = std::max(e, b + 1);
  }
  return run_end;
}

// ---- one batch's select ----------------------------------------------------------------------------------------------
// exact top-k_j lists (serial batches); stale top-(k_j + KMAX) lists (a pipelined run; k_fixup or the replay makes
// them exact); select-ahead top-(k_j + 2 KMAX) lists (k_fixlist makes the Reserve kernel's lists)
enum SelMode { SEL_EXACT, SEL_STALE, SEL_AHEAD };
struct SelectPlan {
  SelMode mode;
  int L, kext;     // list length and the extra entries beyond k_j
  int parts;       // workgroups per pod of an unsharded select (1: one workgroup; DeviceShare batches always)
  bool rc_one;     // the one-workgroup select over [0, N) is register-resident
  bool rc_split;   // ... a part of the split select
  bool sorted;     // the Reserve kernel's lists are in descending key order: they come out of a merge (split or
                   // node-sharded select) or of k_fixlist, not straight out of one k_select workgroup (unordered)
};
// Every site that needs the parts of a batch reads this plan.  Before it existed the sites called select_parts with
// L = the mode's list length (the select itself, k_fixlist's part count) or with 128 (the sortedness of exact and
// stale lists, the k_patch schedule's count of select workgroups): these agree because the exact and stale lengths,
// 64 and 128, both leave 1024 / L >= 8 = the cap of the parts, and the sites that passed 128 never ran for a
// select-ahead batch (L = 192, 1024 / L = 5), whose lists k_fixlist sorts whatever the parts.
// `extra` (an exact-mode batch only): entries beyond k_j -- the remainder of a batch a DSB_CUT stopped inside an open gang
// run, whose rollback may adopt up to `extra` nodes of the run's earlier members as changed slots
inline SelectPlan plan_select(int n_nodes, const Batch& b, SelMode mode, bool sharded, SelectKnob kb, int extra = 0) {
  SelectPlan s;
  s.mode = mode;
  s.L =mode == SEL_AHEAD ? KSTALE2 : mode == SEL_STALE ? KSTALE : KMAX;
  s.kext = mode == SEL_AHEAD ? 2 * KMAX : mode == SEL_STALE ? KMAX : std::min(extra, KMAX - b.pods);
  s.parts = n_nodes > 0 && !b.ds ? select_parts(n_nodes, b.pods, s.L, kb) : 1;
  s.rc_one = select_resident(0, n_nodes);
  s.rc_split = select_resident(0, select_part(0, n_nodes, s.parts));
  s.sorted = mode == SEL_AHEAD || (n_nodes > 0 && !b.ds && (sharded || s.parts > 1));
  return s;
}

// ---- layouts ---------------------------------------------------------------------------------------------------------
struct Take16 {  // consecutive 16-byte aligned parts
  size_t off = 0;
  size_t operator()(size_t bytes) {
    const size_t o = off;
    off = (off + bytes + 15) & ~(size_t)15;
    return o;
  }
};

// The read-back block, device and h_out alike (16-byte aligned parts): scores, placements, the call's error
// word, the fixup stamps [2 nb], the batch end stamps [nb + 1] (st[0]: the call's start), the replay stamps
// [PST nb], the eval start stamps [nb] -- and, not read back, one more eval stamp (a re-run remainder's).
// k_call_begin zeroes the error word and the fixup stamps as one range: [err, st).
// the tail of a call's gang block behind its statuses and tried nodes: ke_debug_gangs' two device
// counters, ke_debug_gang_devices' four from GC_DS, and from GC_STATE the run's state across a DSB_CUT (first position in
// the call, waiting count, satisfied, failed)
constexpr int GC_DS = 2, GC_STATE = 6, GC_WORDS = 10;

struct OutLayout {
  size_t score, chosen, err, fst, st, pst, est, end, total;
  OutLayout(size_t np, size_t nb) {
    Take16 take;
    score = take(4 * np), chosen = take(4 * np), err = take(8), fst = take(16 * nb), st = take(8 * (nb + 1));
    pst = take(8 * PST * nb), est = take(8 * nb);
    end = est + 8 * nb;
    total = est + 8 * (nb + 1);
  }
};

// d_sched (int32 words): ready [n], done [n], T-helper counts [n], select-started counts [n], the Reserve kernels'
// residency flags [n] (by run start), each with a spare word; behind `words` of them the T helpers' lists and
// maxima (THelp), 8-byte aligned.  (The batch bases [n+1] lie in the upload block behind the records and node set
// ids; the error word and the fixup stamps in the read-back block.)
struct SchedLayout {
  int64_t ready, done, tready, sstart, rres, words, tlist, tmx, total;
  explicit SchedLayout(int64_t nb) {
    ready = 0, done = nb + 1, tready = 2 * (nb + 1), sstart = 3 * (nb + 1), rres = 4 * (nb + 1);
    words = (5 * (nb + 1) + 1) & ~1LL;
    tlist = words, tmx = tlist + 2 * (1 + MAX_BATCH);
    total = tmx + 2 * MAX_BATCH;
  }
};

// h_out (page-locked): the read-back block from its first wanted part (the scores lead it, so a call without them
// starts at the placements), then the context's error word and what only some calls have
struct HostOutLayout {
  size_t blk0 = 0, blk_bytes = 0;  // the part of the device block one copy brings
  size_t chosen = 0, score = 0, err = 0, fst = 0, st = 0, pst = 0, est = 0, kerr = 0, dev = 0, cs = 0, vf = 0, numa = 0,
         dcnt = 0, gang = 0, total = 0;
  HostOutLayout() = default;
  // (gangs: the call's gang block -- status [np], tried node [np], GC_WORDS words -- behind everything else)
  HostOutLayout(const OutLayout& ol, size_t np, size_t nb, bool want_score, bool any_ds, bool any_cpu, bool vf_out,
                bool numa_on, bool gangs = false) {
    blk0 = want_score ? ol.score : ol.chosen;
    blk_bytes = ol.end - blk0;
    chosen = ol.chosen - blk0, score = ol.score - blk0, err = ol.err - blk0, fst = ol.fst - blk0;
    st = ol.st - blk0, pst = ol.pst - blk0, est = ol.est - blk0;
    Take16 take{(blk_bytes + 15) & ~(size_t)15};
    kerr = take(4), dev = take(any_ds ? 8 * np : 0), cs = take(any_cpu ? 32 * np : 0);
    vf = take(vf_out ? 2 * DS_MINORS * np : 0), numa = take(numa_on ? 8 * 16 * np : 0);
    dcnt = take(numa_on ? 4 * nb : 0);
    gang = take(gangs ? 4 * (2 * np + GC_WORDS) : 0);
    total = take.off;
  }
};

// ---- the call's statistics -------------------------------------------------------------------------------------------
struct StatsIn {
  const std::vector<Batch>* batches;
  const std::vector<int32_t>* bases;
  const std::vector<int>* run_end;
  int n_pods, n_pipelined;
  const uint64_t *st, *pst, *est, *fst;  // the call's stamps: [nb + 1], [PST nb], [nb], [2 nb]
  const uint32_t* dcnt;                  // deferred BestEffort pairs per batch (n_dcnt of them)
  size_t n_dcnt;
  double span_ms;     // the event-timed span st[0] .. st[nb]
  double sync_ms;     // the call's entry -> the return of its final synchronisation, on the host clock
  uint64_t prev_end;  // the previous call's last batch end stamp (0: none)
  bool behind;        // enqueued behind a call in flight
  int64_t copies, fills;
  bool t_maxima;      // the run's T helpers may deliver maxima (no quota, no k_fixup schedule, helpers on)
  const float* samples;  // sampled (eval, select) event times in ms, n_samples pairs
  int n_samples;
};

// Writes ctx's kstat_*, last_batch_ms, last_pod_lat, call_boundary (Context, or a test's stand-in)
template <class Ctx>
void call_stats(Ctx& ctx, const StatsIn& in) {
  const std::vector<Batch>& batches = *in.batches;
  const int n_batches = (int)batches.size();
  const uint64_t *st = in.st, *pst = in.pst;
  ctx.last_total_ms = in.span_ms;
  ctx.last_pipelined = in.n_pipelined;
  // s_memrealtime ticks -> ms, calibrated against the event-timed span of the whole queue
  const double span = (double)(st[n_batches] - st[0]);
  const double ms_per_tick = span > 0 ? in.span_ms / span : 1e-5;
  // ke_debug_call_boundary: the device time between the previous call's last batch end and this call's first
  // Reserve prologue (a call enqueued behind one in flight; the completions run in submission order)
  ctx.call_boundary[0] = 0;  // (no batch's eval is enqueued ahead of the previous call's end)
  ctx.call_boundary[1] = in.copies;
  ctx.call_boundary[2] = in.fills;
  ctx.call_boundary[3] = in.behind && in.prev_end && pst[0] > in.prev_end
                             ? (int64_t)((double)(pst[0] - in.prev_end) * ms_per_tick * 1e6) : 0;
  ctx.prev_end_tick = st[n_batches];
  // a batch's device service time: from its eval start to the end of its Reserve
  ctx.last_batch_ms.resize(n_batches);
  for (int b = 0; b < n_batches; b++) {
    const uint64_t t0 = std::max(std::min(in.est[b], st[b + 1]), st[0]);
    ctx.last_batch_ms[b] = (double)(st[b + 1] - t0) * ms_per_tick;
  }
  // a pod's latency: from the ke_schedule call's entry (its dequeue) to its batch's Reserve end,
  // the device stamps placed on the host clock by aligning the last one with the return of the final
  // synchronisation (later than the true end: an upper bound)
  ctx.last_pod_lat.resize((size_t)in.n_pods);
  for (int b = 0, p0 = 0; b < n_batches; b++) {  // (a DeviceShare batch cut and re-run covers its first part too)
    const double lat = in.sync_ms - (double)(st[n_batches] - st[b + 1]) * ms_per_tick;
    const int p1 = (*in.bases)[b] + batches[b].pods;
    for (int p = p0; p < p1; p++) ctx.last_pod_lat[(size_t)p] = lat;
    p0 = p1;
  }
  std::vector<char> in_run((size_t)n_batches, 0);  // a pipelined batch after the first of its run
  for (int b = 0; b < n_batches; b++)
    for (int q = b + 1; q < (*in.run_end)[b]; q++) in_run[(size_t)q] = 1;
  // resolve kernel: prologue (candidate/row staging) vs sequential replay; the phases: prologue, then the
  // speculative replay's first round (P, R + S, V), its later rounds, and the write-back (the one-wave replay of
  // other batches, pst[1] <= pst[4], counts entirely as write-back); the first round in detail: T set-up, the
  // prediction loop, wave 1's T rows (concurrent with the loop), wave 0's R; the progressive S of wave 1 (batches
  // with helper T maxima): its polls, record loads + Reserves, rows, and its end after the T set-up
  double pro = 0, loop = 0, ph[6] = {0, 0, 0, 0, 0, 0}, sub[4] = {0, 0, 0, 0}, wv[4] = {0, 0, 0, 0};
  int n_spec = 0, nt = 0, hits = 0, nw = 0;
  // per-batch Reserve time from the in-kernel stamps (start of the batch's prologue -> end of its replay);
  // hand-off = end of batch b-1's replay -> start of batch b (run batches after the first); fixup = k_fixup's
  // workgroup 0 from its wait to its publish
  double res_sum = 0, ho_sum = 0, fx_sum = 0, rows_fetched = 0, rows_changed = 0, spec_rounds = 0;
  int ho_n = 0, fx_n = 0;
  for (int b = 0; b < n_batches; b++) {
    const uint64_t* p = &pst[PST * (size_t)b];
    const bool spec = p[1] > p[4];
    pro += (double)(p[4] - p[0]) * ms_per_tick;
    loop += (double)(st[b + 1] - p[4]) * ms_per_tick;
    ph[0] += (double)(p[4] - p[0]);
    ph[5] += (double)(st[b + 1] - (spec ? p[5] : p[4]));
    if (spec) {
      ph[1] += (double)(p[1] - p[4]);
      ph[2] += (double)(p[2] - p[1]);
      ph[3] += (double)(p[3] - p[2]);
      ph[4] += (double)(p[5] - p[3]);
      n_spec++;
      sub[0] += (double)(p[8] - p[4]);
      sub[1] += (double)(p[9] > p[8] ? p[9] - p[8] : 0);
      sub[2] += (double)(p[10] > p[8] ? p[10] - p[8] : 0);
      sub[3] += (double)(p[11] > p[1] ? p[11] - p[1] : 0);
      const bool t = in.t_maxima && in_run[(size_t)b];
      if (t) nt++, hits += p[12] == 1;
      if (t && p[15] > p[8]) {
        nw++;
        wv[0] += (double)p[13];
        wv[1] += (double)(p[14] & 0xffffffffu);
        wv[2] += (double)(p[14] >> 32);
        wv[3] += (double)(p[15] - p[8]);
      }
    }
    res_sum += (double)(st[b + 1] - p[0]) * ms_per_tick;
    if (in.fst[2 * b + 1] > in.fst[2 * b]) {
      fx_sum += (double)(in.fst[2 * b + 1] - in.fst[2 * b]) * ms_per_tick;
      fx_n++;
    }
    if (in_run[(size_t)b] && p[0] > st[b]) {
      ho_sum += (double)(p[0] - st[b]) * ms_per_tick;
      ho_n++;
    }
    rows_fetched += (double)(p[6] & 0xFFFFFFFFull);
    spec_rounds += (double)(p[6] >> 32);
    rows_changed += (double)p[7];
  }
  ctx.kstat_resolve_prologue_ms = pro / n_batches;
  ctx.kstat_resolve_loop_ms = loop / n_batches;
  for (int i = 0; i < 6; i++) ctx.kstat_resolve_phase_ms[i] = ph[i] * ms_per_tick / n_batches;
  for (int i = 0; i < 4; i++) ctx.kstat_resolve_sub_ms[i] = n_spec ? sub[i] * ms_per_tick / n_spec : 0;
  ctx.kstat_resolve_sub_ms[4] = nt ? (double)hits / nt : 0;
  for (int i = 0; i < 4; i++) ctx.kstat_resolve_wave1_ms[i] = nw ? wv[i] * ms_per_tick / nw : 0;
  ctx.kstat_numa_deferred = 0;
  for (size_t i = 0; i < in.n_dcnt; i++) ctx.kstat_numa_deferred += in.dcnt[i];
  ctx.kstat_resolve_ms = n_batches ? res_sum / n_batches : 0;
  ctx.kstat_spec_failed = n_batches ? spec_rounds / n_batches : 0;
  ctx.kstat_rows_fetched = n_batches ? rows_fetched / n_batches : 0;
  ctx.kstat_rows_changed = n_batches ? rows_changed / n_batches : 0;
  ctx.kstat_fixup_ms = fx_n ? fx_sum / fx_n : 0;
  ctx.kstat_handoff_ms = ho_n ? ho_sum / ho_n : 0;
  ctx.kstat_samples = in.n_samples;
  ctx.kstat_eval_ms = ctx.kstat_select_ms = 0;
  for (int s = 0; s < in.n_samples; s++) {
    ctx.kstat_eval_ms += in.samples[2 * s];
    ctx.kstat_select_ms += in.samples[2 * s + 1];
  }
  if (in.n_samples) {
    ctx.kstat_eval_ms /= in.n_samples;
    ctx.kstat_select_ms /= in.n_samples;
  }
}

}  // namespace ke
