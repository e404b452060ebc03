// The segment plan and the call record (koordinator_amd/csrc/ke_segments.h) compiled alone for the host, for
// tests/test_segments_host.py.  Every mode reads whitespace-separated integers from stdin.
//   segments_check segments   per sequence "n c0 .. c(n-1)" (PodClass bits) one line: "s0 s1 ign alone barrier" per segment
//   segments_check record     per draw "n_segs", then per segment "len cut has_dev has_cs has_vf has_numa" and len + cut
//                             pods of 1 + 4 + 32 + 16 values (minors, cpuset, VF ranks, NUMA amounts): the segment is
//                             filled as a device call's completion fills it, cut = 1 truncates it to len, and it is
//                             appended.  Pods p with p % 7 == 3 are then marked unreserved (chosen -1).  Prints "D n",
//                             then per pod two lines of the same 53 values: through the accessors, and through the flat
//                             views (minors, cpuset, NUMA amounts) with the allocation record's VF ranks; then a line of
//                             the allocation records' node, quota flag, minors, cpuset, NUMA amounts.
//   segments_check restore    "n gen_saved gen_now" and n resv values: a record saved, the live one replaced by another
//                             call's, the saved one restored.  Prints resv, then chosen, uid, quota and the minors.
//   segments_check times      CallTimes over three stand-in segments; prints total_ms, batch_ms, pod_lat.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../koordinator_amd/csrc/ke_segments.h"

using namespace ke;

constexpr int CS = 4, VF = 2 * KE_MAX_MINORS, NUMA = KE_MAX_NUMA * KE_NRES;

static int segments() {
  int32_t n;
  while (std::cin >> n) {
    std::vector<uint8_t> cls((size_t)n);
    for (auto& c : cls) {
      int v;
      std::cin >> v;
      c = (uint8_t)v;
    }
    for (const Segment& s : plan_segments(n, cls.data()))
      printf("%d %d %d %d %d  ", s.s0, s.s1, (int)s.ign, (int)s.alone, (int)s.barrier);
    printf("\n");
  }
  return 0;
}

static void print_pod(uint64_t dev, const uint64_t* cs, const int8_t* vf, const int64_t* numa) {
  printf("%llu", (unsigned long long)dev);
  for (int i = 0; i < CS; i++) printf(" %llu", (unsigned long long)(cs ? cs[i] : 0));
  for (int i = 0; i < VF; i++) printf(" %d", vf ? (int)vf[i] : -1);
  for (int i = 0; i < NUMA; i++) printf(" %lld", (long long)(numa ? numa[i] : 0));
  printf("\n");
}

static int record() {
  int n_segs;
  const std::vector<ke_reservation> no_resv;
  while (std::cin >> n_segs) {
    CallRecords all;
    for (int s = 0; s < n_segs; s++) {
      int len, cut, has[4];
      std::cin >> len >> cut >> has[0] >> has[1] >> has[2] >> has[3];
      const size_t np = (size_t)(len + cut);
      std::vector<uint64_t> dev(np), cs(np * CS);
      std::vector<int8_t> vf(np * VF);
      std::vector<int64_t> numa(np * NUMA);
      for (size_t p = 0; p < np; p++) {
        std::cin >> dev[p];
        for (int i = 0; i < CS; i++) std::cin >> cs[p * CS + i];
        for (int i = 0; i < VF; i++) {
          int v;
          std::cin >> v;
          vf[p * VF + i] = (int8_t)v;
        }
        for (int i = 0; i < NUMA; i++) std::cin >> numa[p * NUMA + i];
      }
      CallRecords seg;
      seg.fill_device(np, dev.data(), has[0], cs.data(), has[1], vf.data(), has[2], numa.data(), has[3]);
      if (seg.n != np) return 1;
      if (cut) seg.truncate((size_t)len);
      all.append(seg, (size_t)len);
    }
    const int32_t n = (int32_t)all.n;
    std::vector<int32_t> chosen((size_t)n);
    std::vector<ke_pod> pods((size_t)n);
    for (int32_t p = 0; p < n; p++) chosen[(size_t)p] = 100 + p, pods[(size_t)p].uid = 1000 + p, pods[(size_t)p].quota = p % 2;
    all.set_pods(n, chosen.data(), pods.data(), true, 0);
    for (int32_t p = 3; p < n; p += 7) all.chosen[(size_t)p] = -1;  // (as ke_unreserve leaves it)
    printf("D %d\n", n);
    const int32_t n_out = n + 2;  // (the views read as absent beyond the call's pods)
    std::vector<uint64_t> fdev((size_t)n_out), fcs((size_t)n_out * CS);
    std::vector<int64_t> fnuma((size_t)n_out * NUMA);
    all.devs.flat(n_out, fdev.data());
    all.cpusets.flat(n_out, fcs.data());
    all.numas.flat(n_out, fnuma.data());
    std::vector<ke_pod_allocation> al;
    for (int32_t p = 0; p < n_out; p++) {
      al.push_back(all.allocation(p, 0, no_resv));
      print_pod(all.dev(p), all.cpuset(p), all.vf(p), all.numa(p));
      // (an unreserved pod's allocation record is blank: its VF ranks are checked on the third line's pods only)
      print_pod(fdev[(size_t)p], &fcs[(size_t)p * CS], al.back().node >= 0 ? &al.back().vf_rank[0][0] : all.vf(p),
                &fnuma[(size_t)p * NUMA]);
    }
    for (const ke_pod_allocation& a : al) {
      printf("%d %d %d ", a.node, (int)a.quota_assigned, (int)a.vf_rank[1][KE_MAX_MINORS - 1]);
      print_pod(a.device_minors, a.cpuset, nullptr, a.numa);
    }
  }
  return 0;
}

static int restore() {
  int n, gen_saved, gen_now;
  std::cin >> n >> gen_saved >> gen_now;
  std::vector<int32_t> chosen((size_t)n);
  std::vector<ke_pod> pods((size_t)n);
  std::vector<uint64_t> dev((size_t)n);
  CallRecords live;
  live.resv.resize((size_t)n);
  for (int p = 0; p < n; p++) {
    std::cin >> live.resv[(size_t)p];
    chosen[(size_t)p] = 10 + p, pods[(size_t)p].uid = 500 + p, pods[(size_t)p].quota = 1, dev[(size_t)p] = 7u + (unsigned)p;
  }
  live.fill_device((size_t)n, dev.data(), true, nullptr, false, nullptr, false, nullptr, false);
  live.set_pods(n, chosen.data(), pods.data(), true, gen_saved);
  CallRecords saved = live;  // (ke_schedule_submit's copy)
  const int32_t other = 1;
  live = CallRecords();
  live.resv.assign(1, 9);
  live.set_pods(1, &other, pods.data(), false, gen_now);  // a later call's records, under the current reservation set
  live.restore(std::move(saved), gen_now);
  if (live.resv_gen != gen_now) return 1;
  for (int32_t r : live.resv) printf("%d ", r);
  printf("\n");
  for (int p = 0; p < n; p++)
    printf("%d %lld %d %llu  ", live.chosen[(size_t)p], (long long)live.uid[(size_t)p], (int)live.quota[(size_t)p],
           (unsigned long long)live.dev(p));
  printf("\n");
  return 0;
}

static int times() {
  CallTimes t;
  t.add(1.5, {0.5, 1.0}, {0.25, 0.5, 0.75});
  t.add(2.25, {}, {});
  t.add(0.125, {2.0}, {4.0});
  printf("%.6f\n", t.total_ms);
  for (double b : t.batch_ms) printf("%.6f ", b);
  printf("\n");
  for (double l : t.pod_lat) printf("%.6f ", l);
  printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "segments") return segments();
  if (mode == "record") return record();
  if (mode == "restore") return restore();
  if (mode == "times") return times();
  return 2;
}
