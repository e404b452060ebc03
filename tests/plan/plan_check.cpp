// The host plan of a ke_schedule call (koordinator_amd/csrc/ke_plan.h) compiled alone for the host: prints what the
// plan computes for the inputs of tests/test_plan_host.py, which compares.  Modes:
//   geometry             the select's parts, part size and wave segments over the test's grid
//   segment   < lines    plan_batches / plan_runs of flag sequences read from stdin
//   layouts              OutLayout, SchedLayout and HostOutLayout for the test's (pods, batches)
//   stats     < stamps   call_stats of hand-made stamps read from stdin
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../koordinator_amd/csrc/ke_plan.h"

using namespace ke;

static int geometry() {
  const int64_t ns[] = {4095, 4096, 8200, 20000, 24575, 24576, 50000, 66061, 140003, 196608, 811264, 1048832};
  const int batches[] = {1, 2, 7, 32, 64};
  const char* knobs[] = {nullptr, "1", "2", "8"};
  const SelMode modes[] = {SEL_EXACT, SEL_STALE, SEL_AHEAD};  // L = 64, 128, 192
  for (int64_t n : ns)
    for (int bp : batches)
      for (const char* kn : knobs)
        for (SelMode m : modes) {
          const Batch b{bp, false, false, false, false};
          const SelectPlan sp = plan_select((int)n, b, m, false, select_knob(kn));
          if (sp.parts != select_parts(n, bp, sp.L, select_knob(kn))) return 1;
          const int part = sp.parts > 1 ? select_part(0, (int)n, sp.parts) : (int)n;
          std::printf("%" PRId64 " %d %s %d %d %d %d %d %d %d", n, bp, kn ? kn : "-", sp.L, sp.kext, sp.parts, part,
                      (int)sp.rc_one, (int)sp.rc_split, (int)sp.sorted);
          for (int p = 0; p < sp.parts; p++) {
            const int lo = std::min<int>((int)n, p * part), hi = std::min<int>((int)n, lo + part);
            std::printf(" %d", select_seg(lo, hi));
          }
          std::printf("\n");
        }
  return 0;
}

// a line: B ds_batch fused n f_0 .. f_{n-1}, f = 1 (PF_DS) | 2 (PF_CPUSET) | 4 (PF_DS_HINT)
// prints: the batches (pods ds cpu cut hint each), then run_end for (pipeline, numa, nodes) =
// (1, 0, 100), (0, 0, 100), (1, 1, 100), (1, 0, 0), each list behind a '|'
static int segment() {
  int B, ds_batch, fused, n;
  while (std::cin >> B >> ds_batch >> fused >> n) {
    std::vector<DevPod> pods((size_t)n);  // (zeroed)
    for (DevPod& p : pods) {
      int f;
      std::cin >> f;
      p.flags = (f & 1 ? PF_DS : 0u) | (f & 2 ? PF_CPUSET : 0u) | (f & 4 ? PF_DS_HINT : 0u);
    }
    const std::vector<Batch> bt = plan_batches(pods.data(), n, B, ds_batch != 0, fused != 0);
    const std::vector<int32_t> bases = plan_bases(bt);
    for (size_t b = 0; b < bt.size(); b++) {
      if (bases[b + 1] - bases[b] != bt[b].pods) return 1;
      std::printf("%d %d %d %d %d ", bt[b].pods, (int)bt[b].ds, (int)bt[b].cpu, (int)bt[b].cut, (int)bt[b].hint);
    }
    const int variants[4][3] = {{1, 0, 100}, {0, 0, 100}, {1, 1, 100}, {1, 0, 0}};
    for (const auto& v : variants) {
      std::printf("|");
      for (int e : plan_runs(bt, v[0] != 0, v[2], v[1] != 0, fused != 0)) std::printf(" %d", e);
    }
    std::printf("\n");
  }
  return 0;
}

static int layouts() {
  const size_t cases[][2] = {{1, 1}, {64, 1}, {5000, 79}, {5000, 5000}};
  for (const auto& c : cases) {
    const OutLayout ol(c[0], c[1]);
    std::printf("out %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", c[0], c[1], ol.score, ol.chosen, ol.err, ol.fst,
                ol.st, ol.pst, ol.est, ol.end, ol.total, OutLayout(c[0], c[0]).total);
    const SchedLayout sl((int64_t)c[1]);
    std::printf("sched %zu %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64
                " %" PRId64 "\n", c[1], sl.ready, sl.done, sl.tready, sl.sstart, sl.rres, sl.words, sl.tlist, sl.tmx, sl.total);
    for (int ws = 0; ws < 2; ws++) {
      const HostOutLayout ho(ol, c[0], c[1], ws != 0, true, true, true, true);
      std::printf("host %zu %zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", c[0], c[1], ws,
                  ho.blk0, ho.blk_bytes, ho.score, ho.chosen, ho.err, ho.fst, ho.st, ho.pst, ho.est, ho.kerr, ho.dev, ho.cs,
                  ho.vf, ho.numa, ho.dcnt, ho.total);
    }
  }
  return 0;
}

// the fields of Context that call_stats writes
struct Stats {
  double last_total_ms = 0;
  int32_t last_pipelined = 0;
  int64_t call_boundary[4] = {0, 0, 0, 0};
  uint64_t prev_end_tick = 0;
  std::vector<double> last_batch_ms, last_pod_lat;
  double kstat_eval_ms = 0, kstat_select_ms = 0, kstat_resolve_ms = 0, kstat_fixup_ms = 0, kstat_handoff_ms = 0;
  double kstat_spec_failed = 0, kstat_rows_fetched = 0, kstat_rows_changed = 0;
  double kstat_resolve_prologue_ms = 0, kstat_resolve_loop_ms = 0;
  double kstat_resolve_phase_ms[6] = {0, 0, 0, 0, 0, 0}, kstat_resolve_sub_ms[5] = {0, 0, 0, 0, 0};
  double kstat_resolve_wave1_ms[4] = {0, 0, 0, 0};
  int64_t kstat_numa_deferred = 0;
  int32_t kstat_samples = 0;
};

template <class T>
static std::vector<T> read_n(size_t n) {
  std::vector<T> v(n);
  for (T& x : v) std::cin >> x;
  return v;
}
static void print(const char* name, const double* v, size_t n) {
  std::printf("%s", name);
  for (size_t i = 0; i < n; i++) std::printf(" %.17g", v[i]);
  std::printf("\n");
}

// stdin: nb n_pods n_pipelined; pods per batch [nb]; run_end [nb]; st [nb + 1]; pst [PST nb]; est [nb]; fst [2 nb];
// dcnt [nb]; span_ms sync_ms prev_end behind copies fills t_maxima; n_samples and 2 n_samples times
static int stats() {
  size_t nb;
  StatsIn in{};
  std::cin >> nb >> in.n_pods >> in.n_pipelined;
  std::vector<Batch> bt;
  for (int p : read_n<int>(nb)) bt.push_back({p, false, false, false, false});
  const std::vector<int32_t> bases = plan_bases(bt);
  const std::vector<int> run_end = read_n<int>(nb);
  const auto st = read_n<uint64_t>(nb + 1), pst = read_n<uint64_t>(PST * nb), est = read_n<uint64_t>(nb),
             fst = read_n<uint64_t>(2 * nb);
  const auto dcnt = read_n<uint32_t>(nb);
  int behind, t_maxima;
  std::cin >> in.span_ms >> in.sync_ms >> in.prev_end >> behind >> in.copies >> in.fills >> t_maxima >> in.n_samples;
  const auto samples = read_n<float>(2 * (size_t)in.n_samples);
  in.batches = &bt, in.bases = &bases, in.run_end = &run_end;
  in.st = st.data(), in.pst = pst.data(), in.est = est.data(), in.fst = fst.data();
  in.dcnt = dcnt.data(), in.n_dcnt = nb;
  in.behind = behind != 0, in.t_maxima = t_maxima != 0, in.samples = samples.data();
  if (!std::cin) return 1;
  Stats s;
  call_stats(s, in);
  const double one[] = {s.last_total_ms, (double)s.last_pipelined, (double)s.prev_end_tick, s.kstat_eval_ms,
                        s.kstat_select_ms, s.kstat_resolve_ms, s.kstat_fixup_ms, s.kstat_handoff_ms, s.kstat_spec_failed,
                        s.kstat_rows_fetched, s.kstat_rows_changed, s.kstat_resolve_prologue_ms, s.kstat_resolve_loop_ms,
                        (double)s.kstat_numa_deferred, (double)s.kstat_samples};
  print("scalars", one, sizeof(one) / sizeof(one[0]));
  const double cb[] = {(double)s.call_boundary[0], (double)s.call_boundary[1], (double)s.call_boundary[2],
                       (double)s.call_boundary[3]};
  print("boundary", cb, 4);
  print("batch_ms", s.last_batch_ms.data(), s.last_batch_ms.size());
  print("pod_lat", s.last_pod_lat.data(), s.last_pod_lat.size());
  print("phase", s.kstat_resolve_phase_ms, 6);
  print("sub", s.kstat_resolve_sub_ms, 5);
  print("wave1", s.kstat_resolve_wave1_ms, 4);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "geometry") return geometry();
  if (mode == "segment") return segment();
  if (mode == "layouts") return layouts();
  if (mode == "stats") return stats();
  std::fprintf(stderr, "usage: plan_check geometry | segment | layouts | stats\n");
  return 2;
}
